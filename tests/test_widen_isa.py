"""CPU tier: the generated code of the widened-sum kernels (reduce_widen.hip,
compiled into the library's last code object, behind the scaled sums' and the
FP8 types').

As tests/test_scale_isa.py does, this test takes the fat binary apart, finds
the code object that holds the widened kernels and points the helpers of
test_kernel_isa / test_f16_isa at it.  For the four ops (bf16, f16, e4m3 and
e5m2 inputs, f32 output) it checks the eight default kernels -- one-shot and
plan (k_reduce_single_scaled, k_reduce_plan_scaled: the plain form runs them
with alpha = 1), TILE 256 x 4 and PHASE 512 x 16, nt and write-through stores.
Each must

  * load its inputs with buffer loads of the NARROW width only: one
    buffer_load_dwordx2 per packet of a 2-byte type, one buffer_load_dword per
    packet of FP8 (four elements either way), and no other buffer load;
  * store with buffer_store_dwordx4 only;
  * keep the descriptors scalar (the v_readfirstlane bound, no waterfall loop
    around a buffer op) and have no private segment;
  * contain no fused multiply-add (v_fma*, v_pk_fma*, v_fmac*, v_mad*): every
    add is an f32 add, and the finishing multiply follows the last add;
  * contain NO narrowing conversion (v_cvt_pk_bf16_f32, v_cvt_f16_f32,
    v_cvt_pk_fp8_f32, v_cvt_pk_bf8_f32): the f32 accumulator is stored as it is;
  * FP8: contain the packed widen of its own format and none of the other's.

The VGPR and instruction counts are printed (DESIGN.md records them), not
asserted.  It skips when the library is not built or the LLVM tools are not
installed.
"""
import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa
import test_ops_isa as opsisa

NS = isa.NS

# name -> (the op's demangled name, the narrow load, the packed widen it must hold or None, the one it must not)
OPS = {
    "bf16": (f"OpWiden<{NS}WidenBF16>", "buffer_load_dwordx2", None, None),
    "f16": (f"OpWiden<{NS}WidenF16>", "buffer_load_dwordx2", "v_cvt_f32_f16", None),
    "e4m3": (f"OpWiden<{NS}WidenF8<0>>", "buffer_load_dword", "v_cvt_pk_f32_fp8", "v_cvt_pk_f32_bf8"),
    "e5m2": (f"OpWiden<{NS}WidenF8<1>>", "buffer_load_dword", "v_cvt_pk_f32_bf8", "v_cvt_pk_f32_fp8"),
}
NARROWING = ("v_cvt_pk_bf16_f32", "v_cvt_f16_f32", "v_cvt_pk_f16_f32", "v_cvt_pkrtz", "v_cvt_pk_fp8_f32",
             "v_cvt_pk_bf8_f32", "v_cvt_sr_")
FUSED = ("v_fma", "v_pk_fma", "v_fmac", "v_mad_mix", "v_mad_f", "v_mac_f", "v_dot")

CASES = [pytest.param(name, i, id=f"{name}-{i}") for name in OPS for i in range(8)]


def kernels_of(op):
    return ([f"k_reduce_single_scaled<{NS}{op}, {s}>" for s in opsisa.shapes(16)] +
            [f"k_reduce_plan_scaled<{NS}{op}, {s}>" for s in opsisa.shapes(16)])


@pytest.fixture(scope="module")
def widen_code_object():
    f16isa.code_object_or_skip()
    original = isa.code_object
    found = None
    try:
        objects = opsisa.code_objects()
        for co in objects:
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("OpWiden<" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the widened-sum kernels"
        assert found == objects[-1] and len(objects) == 4, "the widened kernels live in the fourth unit, linked last"
        yield found
    finally:
        isa.code_object = original
        opsisa.clear_caches()


def test_kernel_set(widen_code_object):
    """Every op has its one-shot and plan kernels and no program kernel; the
    plain kernels (no Scale argument) do not exist for these ops."""
    names = [n for n in isa.kernel_symbols() if "OpWiden<" in n]
    assert not [n for n in names if "k_program" in n], "a program kernel of a widened op"
    assert not [n for n in names if "k_reduce_single<" in n or "k_reduce_plan<" in n], "an unscaled widened kernel"
    for op, _, _, _ in OPS.values():
        for k in kernels_of(op):
            isa.find_symbol(k)


@pytest.mark.parametrize("name,i", CASES)
def test_widened_kernels(widen_code_object, name, i):
    op, load, widen, other = OPS[name]
    kernel = kernels_of(op)[i]
    ins = isa.instructions(kernel)
    ops = [o for _, o, _ in ins]
    loads = sorted({o for o in ops if o.startswith("buffer_load")})
    assert loads == [load], f"{kernel}: buffer loads {loads}, expected {load} only"
    stores = sorted({o for o in ops if o.startswith("buffer_store")})
    assert stores == ["buffer_store_dwordx4"], f"{kernel}: buffer stores {stores}"
    rfl = sum(o.startswith("v_readfirstlane") for o in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    meta = f16isa.metadata_of(kernel)
    print(f"{kernel}: {meta['vgpr_count']} VGPRs, {len(ops)} instructions")
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    fused = sorted({o for o in ops if o.startswith(FUSED)})
    assert not fused, f"{kernel}: fused multiply-adds {fused}"
    narrowing = sorted({o for o in ops if o.startswith(NARROWING)})
    assert not narrowing, f"{kernel}: narrowing conversions {narrowing}"
    assert any(o.startswith(("v_add_f32", "v_pk_add_f32")) for o in ops), f"{kernel}: no f32 add"
    assert any(o.startswith(("v_mul_f32", "v_pk_mul_f32")) for o in ops), f"{kernel}: no finishing f32 multiply"
    if widen:
        assert any(o.startswith(widen) for o in ops), f"{kernel}: no widening {widen}"
    if other:
        wrong = sorted({o for o in ops if o.startswith(other)})
        assert not wrong, f"{kernel}: the other format's conversion {wrong}"
