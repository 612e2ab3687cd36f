"""CPU tier: the generated code of the native fp16 kernels (OpF16).

An fp16 add is one v_pk_add_f16 per two elements, with the accumulator in the
packet's own layout.  This test disassembles the gfx950 code object inside
the built library (tests/test_kernel_isa.py's helpers) and checks, for the
default one-shot and plan kernels of OpF16 (both engines, nt and
write-through stores) and for k_program<OpF16, 2 | 4>, that each

  * passes the descriptor checks bf16's kernels pass (scalar descriptors, no
    waterfall loop around a buffer op),
  * contains v_pk_add_f16 and no v_cvt_ (no widened accumulator),
  * has no private segment (no scratch), and
  * takes no more VGPRs than the OpBF16 kernel of the same shape.

It skips when the library is not built or the LLVM tools are not installed.
"""
import functools
import os
import re

import pytest

import test_kernel_isa as isa

NS = isa.NS
SHAPES = ("256, 4, 11, 0", "256, 4, 31, 0", "512, 16, 11, 1", "512, 16, 31, 1")
KERNELS = ([f"k_reduce_single<{NS}{{op}}, {s}>" for s in SHAPES] + [f"k_reduce_plan<{NS}{{op}}, {s}>" for s in SHAPES] +
           [f"k_program<{NS}{{op}}, {u}>" for u in (2, 4)])


def code_object_or_skip():
    co, why = isa.code_object()
    if co is None:
        pytest.skip(why)
    if not os.path.exists(isa.tool("llvm-readelf")):
        pytest.skip(f"{isa.tool('llvm-readelf')} not installed")
    return co


@functools.lru_cache(maxsize=None)
def kernel_metadata():
    """{mangled kernel name: {field: int}} from the code object's AMDGPU
    metadata note (.vgpr_count, .private_segment_fixed_size, ...)."""
    co, _ = isa.code_object()
    entries = []
    # a kernel's entry opens with "  - .field:", its other top-level fields are indented by four
    for ln in isa.run(isa.tool("llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            entries.append({})
        if entries:
            entries[-1][m.group(2)] = m.group(3).strip("'\"")
    meta = {}
    for e in entries:
        if e.get("symbol", "").endswith(".kd"):
            meta[e["symbol"][:-3]] = {k: int(v) for k, v in e.items() if v.isdigit()}
    return meta


def metadata_of(kernel):
    symbol, _ = isa.find_symbol(kernel)
    m = kernel_metadata().get(symbol)
    assert m and "vgpr_count" in m and "private_segment_fixed_size" in m, f"{kernel}: no metadata found"
    return m


@pytest.mark.parametrize("kernel", KERNELS, ids=[k.format(op="OpF16") for k in KERNELS])
def test_f16_kernels_add_packed_and_stay_narrow(kernel):
    code_object_or_skip()
    f16, bf16 = kernel.format(op="OpF16"), kernel.format(op="OpBF16")
    ins = isa.instructions(f16)
    ops = [op for _, op, _ in ins]
    # the descriptor checks of test_kernel_isa.test_descriptors_stay_scalar
    assert any(op.startswith("buffer_load_dwordx4") for op in ops), f"{f16}: no buffer loads found"
    rfl = sum(op.startswith("v_readfirstlane") for op in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{f16}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{f16}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    # the adds are packed half adds, nothing is widened
    assert "v_pk_add_f16" in ops, f"{f16}: no v_pk_add_f16"
    cvt = sorted({op for op in ops if op.startswith("v_cvt_")})
    assert not cvt, f"{f16}: conversions {cvt}"
    mf, mb = metadata_of(f16), metadata_of(bf16)
    assert mf["private_segment_fixed_size"] == 0, f"{f16}: scratch {mf['private_segment_fixed_size']} B"
    assert mf["vgpr_count"] <= mb["vgpr_count"], f"{f16}: {mf['vgpr_count']} VGPRs, bf16 {mb['vgpr_count']}"
