"""CPU tier: the generated code of the MAX / MIN kernels (reduce_ops.hip).

The library holds two gfx950 code objects, one per kernel translation unit;
tests/test_kernel_isa.py's helpers read the first (reduce.hip, the SUM
kernels).  This test takes the fat binary apart at its bundle marks, finds the
code object that holds the MAX / MIN kernels and points the same helpers at
it.  For the default one-shot and plan kernels (both engines, nt and
write-through stores) and k_program of the twelve ops it checks that each

  * passes the descriptor checks the SUM kernels pass (scalar descriptors, no
    waterfall loop around a buffer op) and has no private segment;
  * f32: contains v_maximum3_f32 / v_minimum3_f32;
  * f16: contains v_pk_maximum3_f16 / v_pk_minimum3_f16 and no v_cvt_;
  * bf16: contains no v_cvt_pk_bf16_f32 (nothing rounds);
  * f32, bf16, f16: takes no more VGPRs than the SUM kernel of the same shape.

It skips when the library is not built or the LLVM tools are not installed.
"""
import os
import tempfile

import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa

NS = isa.NS
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

# kind -> (the op's demangled template name with {b} = true (MAX) / false (MIN), PHASE packets per lane, SUM op)
OPS = {
    "f32": ("OpFloatMM<{b}, float, float vector[4]>", 16, "OpF32"),
    "f64": ("OpFloatMM<{b}, double, double vector[2]>", 16, None),
    "bf16": ("OpBF16MM<{b}>", 16, "OpBF16"),
    "f16": ("OpFloatMM<{b}, _Float16, _Float16 vector[8]>", 16, "OpF16"),
    "i32": ("OpIntMM<{b}, int, int vector[4]>", 8, None),
    "u64": ("OpIntMM<{b}, unsigned long, unsigned long vector[2]>", 16, None),
}


def shapes(p):
    return ("256, 4, 11, 0", "256, 4, 31, 0", f"512, {p}, 11, 1", f"512, {p}, 31, 1")


def kernels_of(op, p):
    """Demangled-name fragments of an op's default kernels."""
    return ([f"k_reduce_single<{NS}{op}, {s}>" for s in shapes(p)] + [f"k_reduce_plan<{NS}{op}, {s}>" for s in shapes(p)] +
            [f"k_program<{NS}{op}, 4>"])


CASES = [pytest.param(kind, mx, i, id=f"{kind}-{'max' if mx else 'min'}-{i}")
         for kind in OPS for mx in (True, False) for i in range(9)]


def code_objects():
    """Every gfx950 code object of the library, one per bundle of its .hip_fatbin."""
    tmp = tempfile.mkdtemp(prefix="hiccl_ops_isa_")
    fat = os.path.join(tmp, "fat.bin")
    isa.run(isa.tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", isa.LIB, os.path.join(tmp, "rest"))
    data = open(fat, "rb").read()
    starts, at = [], data.find(MAGIC)
    while at >= 0:
        starts.append(at)
        at = data.find(MAGIC, at + 1)
    out = []
    for i, s in enumerate(starts):
        piece, co = os.path.join(tmp, f"bundle{i}.bin"), os.path.join(tmp, f"bundle{i}.co")
        with open(piece, "wb") as fh:
            fh.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        isa.run(isa.tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={piece}",
                f"--targets={isa.TARGET}", f"--output={co}")
        out.append(co)
    return out


def clear_caches():
    isa.kernel_symbols.cache_clear()
    f16isa.kernel_metadata.cache_clear()


@pytest.fixture(scope="module")
def ops_code_object():
    """Points the helpers of test_kernel_isa / test_f16_isa at the MAX / MIN
    code object for this module; yields the VGPR counts of the SUM kernels."""
    f16isa.code_object_or_skip()
    sum_vgprs = {}
    for kind, (_, p, sum_op) in OPS.items():
        if sum_op:
            for k in kernels_of(sum_op, p):
                sum_vgprs[k] = f16isa.metadata_of(k)["vgpr_count"]
    original = isa.code_object
    found = None
    try:
        for co in code_objects():
            isa.code_object = lambda co=co: (co, "")
            clear_caches()
            if any("MM<" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the MAX / MIN kernels"
        yield sum_vgprs
    finally:
        isa.code_object = original
        clear_caches()


@pytest.mark.parametrize("kind,mx,i", CASES)
def test_ops_kernels(ops_code_object, kind, mx, i):
    tmpl, p, sum_op = OPS[kind]
    op = tmpl.format(b="true" if mx else "false")
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
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    word = "maximum3" if mx else "minimum3"
    if kind == "f32":
        assert f"v_{word}_f32" in ops, f"{kernel}: no v_{word}_f32"
    if kind == "f16":
        assert f"v_pk_{word}_f16" in ops, f"{kernel}: no v_pk_{word}_f16"
        cvt = sorted({o for o in ops if o.startswith("v_cvt_")})
        assert not cvt, f"{kernel}: conversions {cvt}"
    if kind == "bf16":
        assert "v_cvt_pk_bf16_f32" not in ops, f"{kernel}: a rounding conversion in an exact op"
    if sum_op:
        sum_kernel = kernels_of(sum_op, p)[i]
        assert meta["vgpr_count"] <= ops_code_object[sum_kernel], \
            f"{kernel}: {meta['vgpr_count']} VGPRs, {sum_kernel} {ops_code_object[sum_kernel]}"
