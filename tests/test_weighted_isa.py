"""CPU tier: the generated code of the weighted widened-sum kernels
(reduce_weighted.hip, compiled into the library's last code object behind the
mixed plan kernels).

Modelled on tests/test_widen_isa.py and tests/test_accum_isa.py, whose helpers
and lists it uses.  For the eight ops -- bf16, f16, e4m3 and e5m2 inputs, f32
output, overwriting (OpWeighted) and accumulating (OpWeightedAccum) -- the
eight default kernels are checked: one-shot and plan (k_reduce_single_weighted,
k_reduce_plan_weighted), TILE 256 x 4 and PHASE 512 x P (P = 16 overwriting, 8
accumulating), nt and write-through stores.  Each must

  * load its inputs with buffer loads of the type's NARROW width only, plus,
    accumulating, buffer_load_dwordx4 (the old output) and nothing else;
  * store with buffer_store_dwordx4 only;
  * keep the descriptors scalar (the v_readfirstlane bound, no waterfall loop
    around a buffer op) and have no private segment;
  * contain NO fused multiply-add of any spelling: the product w * x and the
    add that follows it are two separately rounded f32 operations;
  * contain at least one f32 multiply and one f32 add;
  * FP8: contain the packed widen of its own format and none of the other's;
  * contain no narrowing conversion.

The library still has four code objects with these kernels in the last one.
The VGPR and instruction counts are printed (DESIGN.md records them), not
asserted.  It skips when the library is not built or the LLVM tools are not
installed.
"""
import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa
import test_ops_isa as opsisa
import test_widen_isa as widenisa

NS = isa.NS

WIDENINGS = {
    "bf16": ("WidenBF16", "buffer_load_dwordx2", None, None),
    "f16": ("WidenF16", "buffer_load_dwordx2", "v_cvt_f32_f16", None),
    "e4m3": ("WidenF8<0>", "buffer_load_dword", "v_cvt_pk_f32_fp8", "v_cvt_pk_f32_bf8"),
    "e5m2": ("WidenF8<1>", "buffer_load_dword", "v_cvt_pk_f32_bf8", "v_cvt_pk_f32_fp8"),
}
# family -> (the op template, packets per lane of its PHASE chunk, does it read the old output)
FAMILIES = {"over": ("OpWeighted", 16, False), "accum": ("OpWeightedAccum", 8, True)}
OLD_OUTPUT_LOAD = "buffer_load_dwordx4"


def op_name(family, kind):
    return f"{FAMILIES[family][0]}<{NS}{WIDENINGS[kind][0]}>"


def kernels_of(family, kind):
    op, p = op_name(family, kind), FAMILIES[family][1]
    return ([f"k_reduce_single_weighted<{NS}{op}, {s}>" for s in opsisa.shapes(p)] +
            [f"k_reduce_plan_weighted<{NS}{op}, {s}>" for s in opsisa.shapes(p)])


CASES = [pytest.param(family, kind, i, id=f"{family}-{kind}-{i}")
         for family in FAMILIES for kind in WIDENINGS for i in range(8)]


@pytest.fixture(scope="module")
def weighted_code_object():
    f16isa.code_object_or_skip()
    original = isa.code_object
    found = None
    try:
        objects = opsisa.code_objects()
        for co in objects:
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("OpWeighted<" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the weighted widened-sum kernels"
        assert found == objects[-1] and len(objects) == 4, "the weighted kernels live in the fourth unit, linked last"
        yield found
    finally:
        isa.code_object = original
        opsisa.clear_caches()


def test_kernel_set(weighted_code_object):
    """Every op has its one-shot and plan kernels and nothing else: no program
    kernel, and none of the unweighted kernels' entry points."""
    symbols = isa.kernel_symbols()
    names = [n for n in symbols if "OpWeighted<" in n or "OpWeightedAccum<" in n]
    assert not [n for n in names if "k_program" in n], "a program kernel of a weighted op"
    other = [n for n in names if "k_reduce_single_weighted<" not in n and "k_reduce_plan_weighted<" not in n]
    assert not other, f"a weighted op in another kernel: {other[:3]}"
    assert any("OpWiden<" in n for n in symbols) and any("OpWidenAccum<" in n for n in symbols)
    for family in FAMILIES:
        for kind in WIDENINGS:
            for k in kernels_of(family, kind):
                isa.find_symbol(k)
    # per op: 4 one-shot kernels, and the 4 plan kernels again with peer (system-scope) loads
    assert len(names) == 8 * 12, f"{len(names)} weighted kernels, expected 96"


@pytest.mark.parametrize("family,kind,i", CASES)
def test_weighted_kernels(weighted_code_object, family, kind, i):
    _, load, widen, other = WIDENINGS[kind]
    accum = FAMILIES[family][2]
    kernel = kernels_of(family, kind)[i]
    ins = isa.instructions(kernel)
    ops = [o for _, o, _ in ins]
    loads = sorted({o for o in ops if o.startswith("buffer_load")})
    expected = sorted([load, OLD_OUTPUT_LOAD]) if accum else [load]
    assert loads == expected, f"{kernel}: buffer loads {loads}, expected {expected}"
    stores = sorted({o for o in ops if o.startswith("buffer_store")})
    assert stores == ["buffer_store_dwordx4"], f"{kernel}: buffer stores {stores}"
    rfl = sum(o.startswith("v_readfirstlane") for o in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    meta = f16isa.metadata_of(kernel)
    muls = sum(o.startswith(("v_mul_f32", "v_pk_mul_f32")) for o in ops)
    adds = sum(o.startswith(("v_add_f32", "v_pk_add_f32")) for o in ops)
    print(f"{kernel}: {meta['vgpr_count']} VGPRs, {len(ops)} instructions, {muls} f32 multiplies, {adds} f32 adds")
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    fused = sorted({o for o in ops if o.startswith(widenisa.FUSED)})
    assert not fused, f"{kernel}: fused multiply-adds {fused}"
    narrowing = sorted({o for o in ops if o.startswith(widenisa.NARROWING)})
    assert not narrowing, f"{kernel}: narrowing conversions {narrowing}"
    assert adds, f"{kernel}: no f32 add"
    assert muls, f"{kernel}: no f32 multiply"
    if widen:
        assert any(o.startswith(widen) for o in ops), f"{kernel}: no widening {widen}"
    if other:
        wrong = sorted({o for o in ops if o.startswith(other)})
        assert not wrong, f"{kernel}: the other format's conversion {wrong}"
