"""CPU tier: the generated code of the mixed plan kernels (reduce_mixed.hip:
k_reduce_plan_mixed, a scaled plan whose computes are scaled one by one).

Built on the helpers tests/test_scale_isa.py uses: the library's last code
object holds the scaled kernels and, behind them, the mixed ones.  For every
mixed plan kernel -- the ten scaled ops (f32, f64, bf16 and f16 native and
wide, e4m3 and e5m2 native and wide), both engines' default shapes, nt and
write-through stores, default and peer loads -- it checks that the kernel

  * passes the descriptor checks the SUM kernels pass (buffer loads, scalar
    descriptors, no waterfall loop around a buffer op);
  * has no private segment;
  * falls into no lower occupancy step than the scaled plan kernel of the same
    shape (test_scale_isa.waves_per_simd);
  * f32 and f64: holds no fused multiply-add on floats;
  * native f16: holds no v_fma_mix* and no v_pk_mul_f16.

It skips when the library is not built or the LLVM tools are not installed.
"""
import pytest

import test_f16_isa as f16isa
import test_kernel_isa as isa
import test_ops_isa as opsisa
from test_prod_isa import fused_float
from test_scale_isa import OPS as SCALE_OPS, waves_per_simd

NS = isa.NS

# name -> (the scaled op's demangled name, PHASE packets per lane, what it is)
OPS = {name: (op, p, what) for name, (op, _, p, what) in SCALE_OPS.items()}
for _f, _fmt in ((0, "e4m3"), (1, "e5m2")):
    OPS[_fmt] = (f"OpF8Scaled<{NS}OpF8<{_f}>, {_f}>", 16, "f8")
    OPS[_fmt + "-wide"] = (f"OpF8Scaled<{NS}OpF8Wide<{_f}>, {_f}>", 8, "f8")

POLS = (11, 31, 12, 32)  # 10 * store + load: nt / write-through stores, nt / system-scope (peer) loads


def shapes(p):
    return [f"256, 4, {pol}, 0" for pol in POLS] + [f"512, {p}, {pol}, 1" for pol in POLS]


CASES = [pytest.param(name, i, id=f"{name}-{i}") for name in OPS for i in range(2 * len(POLS))]


@pytest.fixture(scope="module")
def mixed_code_object():
    """Points the helpers at the code object that holds the mixed kernels: the
    scaled sums', the library's fourth and last."""
    f16isa.code_object_or_skip()
    original = isa.code_object
    found = None
    try:
        objects = opsisa.code_objects()
        for co in objects:
            isa.code_object = lambda co=co: (co, "")
            opsisa.clear_caches()
            if any("k_reduce_plan_mixed" in name for name in isa.kernel_symbols()):
                found = co
                break
        assert found, "no code object of the library holds the mixed plan kernels"
        assert found == objects[-1] and len(objects) == 4, "the mixed kernels live in the scaled unit, linked last"
        assert any("k_reduce_plan_scaled" in name for name in isa.kernel_symbols())
        yield found
    finally:
        isa.code_object = original
        opsisa.clear_caches()


def test_exactly_the_shapes_of_the_scaled_plan_kernels(mixed_code_object):
    """80 mixed kernels: 10 ops x 2 engines x 4 policies, no tuned shape."""
    names = [n for n in isa.kernel_symbols() if "k_reduce_plan_mixed" in n]
    assert len(names) == len(OPS) * 2 * len(POLS), len(names)


@pytest.mark.parametrize("name,i", CASES)
def test_mixed_kernels(mixed_code_object, name, i):
    op, p, what = OPS[name]
    kernel = f"k_reduce_plan_mixed<{NS}{op}, {shapes(p)[i]}>"
    scaled_kernel = f"k_reduce_plan_scaled<{NS}{op}, {shapes(p)[i]}>"
    ins = isa.instructions(kernel)
    ops = [o for _, o, _ in ins]
    # the descriptor checks of test_kernel_isa.test_descriptors_stay_scalar
    assert any(o.startswith("buffer_load_dwordx4") for o in ops), f"{kernel}: no buffer loads found"
    rfl = sum(o.startswith("v_readfirstlane") for o in ops)
    assert rfl <= isa.MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = isa.waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
    meta = f16isa.metadata_of(kernel)
    scaled_v = f16isa.metadata_of(scaled_kernel)["vgpr_count"]
    print(f"{kernel}: {meta['vgpr_count']} VGPRs (scaled: {scaled_v}), {len(ops)} instructions")
    assert meta["private_segment_fixed_size"] == 0, f"{kernel}: scratch {meta['private_segment_fixed_size']} B"
    assert waves_per_simd(meta["vgpr_count"]) >= waves_per_simd(scaled_v), \
        f"{kernel}: {meta['vgpr_count']} VGPRs is a lower occupancy step than {scaled_kernel}'s {scaled_v}"
    if what in ("fmul32", "fmul64"):
        fused = sorted({o for o in ops if fused_float(o)})
        assert not fused, f"{kernel}: fused multiply-adds {fused}"
    if what == "f16":
        mix = sorted({o for o in ops if o.startswith("v_fma_mix")})
        assert not mix, f"{kernel}: {mix}: the finishing multiply merged with a conversion"
        assert "v_pk_mul_f16" not in ops, f"{kernel}: a half multiply in the finishing step"
