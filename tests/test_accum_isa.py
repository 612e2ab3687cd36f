"""CPU tier: the generated code of the accumulating widened-sum kernels
(reduce_accum.hip, compiled into the library's last code object behind the
widened sums').

Modelled on tests/test_widen_isa.py, whose helpers and lists it uses: the fat
binary is taken apart, the code object that holds the kernels found, and for the
four ops (bf16, f16, e4m3 and e5m2 inputs, f32 output, out = out + alpha * sum)
the eight default kernels checked -- one-shot and plan (k_reduce_single_scaled,
k_reduce_plan_scaled: the plain form runs them with alpha = 1), TILE 256 x 4 and
PHASE 512 x 8 (the half chunk: the old output's packets are held next to the
accumulators, and at 16 packets per lane the bf16 kernel spilled), nt and
write-through stores.  Each must

  * load with buffer loads of the type's NARROW width (the inputs) and
    buffer_load_dwordx4 (the old output, through the store's descriptor), and
    nothing else;
  * store with buffer_store_dwordx4 only;
  * keep the descriptors scalar (the v_readfirstlane bound, no waterfall loop
    around a buffer op) and have no private segment;
  * contain NO fused multiply-add: the sum, the scale and the add of the old
    output are three separately rounded f32 operations;
  * contain no narrowing conversion;
  * contain an f32 add and an f32 multiply.

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

# name -> (the op's demangled name, the narrow load of its inputs)
OPS = {
    "bf16": (f"OpWidenAccum<{NS}WidenBF16>", "buffer_load_dwordx2"),
    "f16": (f"OpWidenAccum<{NS}WidenF16>", "buffer_load_dwordx2"),
    "e4m3": (f"OpWidenAccum<{NS}WidenF8<0>>", "buffer_load_dword"),
    "e5m2": (f"OpWidenAccum<{NS}WidenF8<1>>", "buffer_load_dword"),
}
OLD_OUTPUT_LOAD = "buffer_load_dwordx4"

PHASE_P = 8  # packets per lane of these ops' PHASE chunk


def kernels_of(op):
    return ([f"k_reduce_single_scaled<{NS}{op}, {s}>" for s in opsisa.shapes(PHASE_P)] +
            [f"k_reduce_plan_scaled<{NS}{op}, {s}>" for s in opsisa.shapes(PHASE_P)])


CASES = [pytest.param(name, i, id=f"{name}-{i}") for name in OPS for i in range(8)]


@pytest.fixture(scope="module")
def accum_code_object():
    f16isa.code_object_or_skip()
    original = isa.code_object
    found = None
    try:
        objects = opsisa.code_objects()
        for co in objects:
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("OpWidenAccum<" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the accumulating widened-sum kernels"
        assert found == objects[-1] and len(objects) == 4, "the accumulating kernels live in the fourth unit, linked last"
        yield found
    finally:
        isa.code_object = original
        opsisa.clear_caches()


def test_kernel_set(accum_code_object):
    """Every op has its one-shot and plan kernels and no program kernel; the
    plain kernels (no Scale argument) do not exist for these ops; the widened
    sums' kernels sit in the same code object."""
    symbols = isa.kernel_symbols()
    names = [n for n in symbols if "OpWidenAccum<" in n]
    assert not [n for n in names if "k_program" in n], "a program kernel of an accumulating op"
    assert not [n for n in names if "k_reduce_single<" in n or "k_reduce_plan<" in n], "an unscaled accumulating kernel"
    assert any("OpWiden<" in n for n in symbols), "the widened kernels are not in the last code object"
    for op, _ in OPS.values():
        for k in kernels_of(op):
            isa.find_symbol(k)


@pytest.mark.parametrize("name,i", CASES)
def test_accumulating_kernels(accum_code_object, name, i):
    op, load = OPS[name]
    kernel = kernels_of(op)[i]
    ins = isa.instructions(kernel)
    ops = [o for _, o, _ in ins]
    loads = sorted({o for o in ops if o.startswith("buffer_load")})
    assert loads == sorted([load, OLD_OUTPUT_LOAD]), f"{kernel}: buffer loads {loads}, expected {load} and {OLD_OUTPUT_LOAD}"
    stores = sorted({o for o in ops if o.startswith("buffer_store")})
    assert stores == ["buffer_store_dwordx4"], f"{kernel}: buffer stores {stores}"
    rfl = sum(o.startswith("v_readfirstlane") for o in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    meta = f16isa.metadata_of(kernel)
    print(f"{kernel}: {meta['vgpr_count']} VGPRs, {len(ops)} instructions")
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    fused = sorted({o for o in ops if o.startswith(widenisa.FUSED)})
    assert not fused, f"{kernel}: fused multiply-adds {fused}"
    narrowing = sorted({o for o in ops if o.startswith(widenisa.NARROWING)})
    assert not narrowing, f"{kernel}: narrowing conversions {narrowing}"
    assert any(o.startswith(("v_add_f32", "v_pk_add_f32")) for o in ops), f"{kernel}: no f32 add"
    assert any(o.startswith(("v_mul_f32", "v_pk_mul_f32")) for o in ops), f"{kernel}: no f32 multiply"
