"""CPU tier: the generated code of the PROD and bitwise kernels (reduce_prod.hip).

The library holds three gfx950 code objects, one per kernel translation unit.
As tests/test_ops_isa.py does for MAX / MIN, this test takes the fat binary
apart, finds the code object that holds the new kernels (by an op's name) and
points the helpers of test_kernel_isa / test_f16_isa at it.  For the default
one-shot and plan kernels (both engines, nt and write-through stores) and
k_program of the twelve ops it checks that each

  * passes the descriptor checks the SUM kernels pass (buffer loads, scalar
    descriptors, no waterfall loop around a buffer op) and has no private
    segment;
  * f32 PROD: contains v_pk_mul_f32 or v_mul_f32 and no fused multiply-add on
    floats (v_fma*, v_pk_fma*, v_fmac*, v_mad* / v_mac* on floats); f64 PROD
    likewise with v_mul_f64;
  * f16 PROD: contains v_pk_mul_f16 and no v_cvt_;
  * bf16 PROD: contains v_cvt_pk_bf16_f32 (it rounds after every multiply);
  * int32 / uint64 PROD: contains an integer multiply;
  * BAND / BOR / BXOR: contains the matching v_and* / v_or* / v_xor*;
  * f32 and f16 PROD: takes no more VGPRs than the SUM kernel of the same
    shape (the structure is identical).

The VGPR counts of bf16, f64 and the integers have no bound beyond "no
scratch"; DESIGN.md section 4 records them.  It skips when the library is not
built or the LLVM tools are not installed.
"""
import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa
import test_ops_isa as opsisa

kernels_of = opsisa.kernels_of

# name -> (the op's demangled name, PHASE packets per lane, the SUM op bounding its VGPRs, what it is)
OPS = {
    "prod-f32": ("OpFloatProd<float, float vector[4]>", 16, "OpF32", "fmul32"),
    "prod-f64": ("OpFloatProd<double, double vector[2]>", 16, None, "fmul64"),
    "prod-bf16": ("OpBF16Prod", 16, None, "bf16"),
    "prod-f16": ("OpFloatProd<_Float16, _Float16 vector[8]>", 16, "OpF16", "f16"),
    "prod-i32": ("OpIntFold<0, unsigned int, unsigned int vector[4]>", 8, None, "imul"),
    "prod-u64": ("OpIntFold<0, unsigned long, unsigned long vector[2]>", 16, None, "imul"),
    "band-i32": ("OpIntFold<1, unsigned int, unsigned int vector[4]>", 8, None, "v_and"),
    "band-u64": ("OpIntFold<1, unsigned long, unsigned long vector[2]>", 16, None, "v_and"),
    "bor-i32": ("OpIntFold<2, unsigned int, unsigned int vector[4]>", 8, None, "v_or"),
    "bor-u64": ("OpIntFold<2, unsigned long, unsigned long vector[2]>", 16, None, "v_or"),
    "bxor-i32": ("OpIntFold<3, unsigned int, unsigned int vector[4]>", 8, None, "v_xor"),
    "bxor-u64": ("OpIntFold<3, unsigned long, unsigned long vector[2]>", 16, None, "v_xor"),
}

CASES = [pytest.param(name, i, id=f"{name}-{i}") for name in OPS for i in range(9)]


def fused_float(o):
    """A fused or multiply-add instruction on floating operands."""
    if o.startswith(("v_fma", "v_pk_fma", "v_fmac", "v_dot")):
        return True
    return o.startswith(("v_mad", "v_mac", "v_pk_mad")) and ("_f" in o or "mix" in o or "legacy" in o)


@pytest.fixture(scope="module")
def prod_code_object():
    """Points the helpers at the PROD / bitwise code object for this module;
    yields the VGPR counts of the SUM kernels."""
    f16isa.code_object_or_skip()
    sum_vgprs = {}
    for _, p, sum_op, _ in OPS.values():
        if sum_op:
            for k in kernels_of(sum_op, p):
                sum_vgprs[k] = f16isa.metadata_of(k)["vgpr_count"]
    original = isa.code_object
    found = None
    try:
        for co in opsisa.code_objects():
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("OpBF16Prod" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the PROD kernels"
        yield sum_vgprs
    finally:
        isa.code_object = original
        opsisa.clear_caches()


@pytest.mark.parametrize("name,i", CASES)
def test_prod_kernels(prod_code_object, name, i):
    op, p, sum_op, what = OPS[name]
    kernel = kernels_of(op, p)[i]
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
    if what in ("fmul32", "fmul64"):
        muls = ("v_pk_mul_f32", "v_mul_f32") if what == "fmul32" else ("v_mul_f64",)
        assert any(o.startswith(muls) for o in ops), f"{kernel}: none of {muls}"
        fused = sorted({o for o in ops if fused_float(o)})
        assert not fused, f"{kernel}: fused multiply-adds {fused}"
    elif what == "f16":
        assert any(o.startswith("v_pk_mul_f16") for o in ops), f"{kernel}: no v_pk_mul_f16"
        cvt = sorted({o for o in ops if o.startswith("v_cvt_")})
        assert not cvt, f"{kernel}: conversions {cvt}"
    elif what == "bf16":
        assert "v_cvt_pk_bf16_f32" in ops, f"{kernel}: no v_cvt_pk_bf16_f32: the product is not rounded per multiply"
        assert any(o.startswith(("v_mul_f32", "v_pk_mul_f32")) for o in ops), f"{kernel}: no f32 multiply"
    elif what == "imul":
        assert any(o.startswith(("v_mul_lo_u32", "v_mad_u64_u32")) for o in ops), f"{kernel}: no integer multiply"
    else:
        assert any(o.startswith(what) for o in ops), f"{kernel}: no {what}*"
    if sum_op:
        sum_kernel = kernels_of(sum_op, p)[i]
        assert meta["vgpr_count"] <= prod_code_object[sum_kernel], \
            f"{kernel}: {meta['vgpr_count']} VGPRs, {sum_kernel} {prod_code_object[sum_kernel]}"
