"""CPU tier of the per-compute "unscaled" flag (hiccl_reduce_plan_add_unscaled,
hiccl_reduce_plan_num_unscaled): the ABI's declarations, the refusals and the
counting, through ctypes as tests/test_widen_cpu.py does -- before any device
work: the pointers here are not device memory and nothing is launched.  (A plan
binds to a device when it is created: the plan tests skip where there is none.)
"""
import ctypes

import pytest
import torch

import hiccl_amd
from hiccl_amd import _lib as L
from test_widen_cpu import _plan, _refused, _tab

NEW_SYMBOLS = ("hiccl_reduce_plan_add_unscaled", "hiccl_reduce_plan_num_unscaled")
FLOATS = (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_BFLOAT16, L.HICCL_FLOAT16, L.HICCL_FLOAT8_E4M3, L.HICCL_FLOAT8_E5M2)
NARROW = (L.HICCL_BFLOAT16, L.HICCL_FLOAT16, L.HICCL_FLOAT8_E4M3, L.HICCL_FLOAT8_E5M2)


def _add(lib, h, out, ins, count, unscaled):
    fn = lib.hiccl_reduce_plan_add_unscaled if unscaled else lib.hiccl_reduce_plan_add
    return fn(h, ctypes.c_void_p(out), _tab(list(ins)), len(ins), count)


def test_new_symbols_are_declared_bound_and_exported():
    declared = L.header_functions()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L._SIGS and hasattr(L.lib(), name), name
    assert L.lib().hiccl_version() >= 900  # 0.8.0 scaled every compute of a plan or none
    lib = L.lib()
    assert lib.hiccl_reduce_plan_num_unscaled(None) == 0
    _refused(lib.hiccl_reduce_plan_add_unscaled(None, ctypes.c_void_p(0x100000), _tab([0x200000]), 1, 4),
             "plan_add_unscaled", "plan is NULL")


def test_python_layer_refuses_an_unscaled_compute_on_a_widened_plan():
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        pytest.skip("no HIP device to bind a plan to")
    comp = hiccl_amd.Compute(torch.bfloat16, device=0, out_dtype=torch.float32)
    try:
        t = torch.empty(0)
        with pytest.raises(ValueError, match="no unscaled compute"):
            comp.add([t], t, 4, compid=0, unscaled=True)
        comp.add([t], t, 4, compid=1, unscaled=True)  # another rank's compute: not recorded, as ever
        assert comp.num_unscaled() == 0
    finally:
        comp.close()


@pytest.mark.parametrize("dt", FLOATS)
def test_num_unscaled_counts_and_the_flag_outlives_the_scale(dt):
    lib = L.lib()
    h = _plan(dt)
    alpha, got = ctypes.c_double(0.7), ctypes.c_double()
    try:
        assert lib.hiccl_reduce_plan_num_unscaled(h) == 0
        # without a scale it is hiccl_reduce_plan_add: the same buffer rules, the same no-op at count 0
        assert _add(lib, h, 0x100000, (0x200000, 0x300000), 100, True) == 0, L.last_error()
        assert _add(lib, h, 0x400000, (0x500000,), 0, True) == 0
        _refused(_add(lib, h, 0, (0x200000,), 4, True), "out is NULL")
        _refused(_add(lib, h, 0x100000, (0,), 4, True), "in[0] is NULL")
        assert lib.hiccl_reduce_plan_num_unscaled(h) == 1 and lib.hiccl_reduce_plan_numcomp(h) == 1
        assert _add(lib, h, 0x600000, (0x700000,), 7, False) == 0
        assert lib.hiccl_reduce_plan_num_unscaled(h) == 1 and lib.hiccl_reduce_plan_numcomp(h) == 2
        # set, change and clear the scale: the flags stay
        for a in (0.7, 0.25, None, 0.0):
            assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(ctypes.c_double(a)) if a is not None else None) == 0
            assert lib.hiccl_reduce_plan_num_unscaled(h) == 1
            assert lib.hiccl_reduce_plan_scale(h, ctypes.byref(got)) == (0 if a is None else 1)
        assert _add(lib, h, 0x800000, (0x900000, 0xa00000, 0xb00000), 33, True) == 0
        assert lib.hiccl_reduce_plan_num_unscaled(h) == 2 and lib.hiccl_reduce_plan_numcomp(h) == 3
        esz = lib.hiccl_dtype_size(dt)
        assert lib.hiccl_reduce_plan_bytes(h) == (100 * 3 + 7 * 2 + 33 * 4) * esz  # the flag prices nothing
        # a scaled plan -- mixed here -- keeps refusing the shapes the scaled kernels lack, and another operator
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(alpha)) == 0
        cfg = L.ReduceConfig(engine=L.HICCL_ENGINE_TILE, unroll=2)
        _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)), "plan_set_config")
        _refused(lib.hiccl_reduce_plan_set_op(h, L.HICCL_OP_MAX), "plan_set_op", "scaled plan")
    finally:
        lib.hiccl_reduce_plan_destroy(h)


def test_a_scaled_plan_of_unscaled_computes_alone_keeps_the_scaled_shapes():
    """Every compute unscaled: the launches take the plain SUM kernels, but a
    scaled compute may come later, so the config stays one the scaled kernels have."""
    lib = L.lib()
    h = _plan(L.HICCL_FLOAT32)
    try:
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(ctypes.c_double(0.5))) == 0
        assert _add(lib, h, 0x100000, (0x200000, 0x300000), 100, True) == 0
        cfg = L.ReduceConfig(engine=L.HICCL_ENGINE_TILE, unroll=8)
        _refused(lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)), "plan_set_config")
        assert lib.hiccl_reduce_plan_set_scale(h, None) == 0
        assert lib.hiccl_reduce_plan_set_config(h, ctypes.byref(cfg)) == 0, L.last_error()  # a plain f32 plan has it
    finally:
        lib.hiccl_reduce_plan_destroy(h)


@pytest.mark.parametrize("dt", NARROW)
def test_widened_and_accumulating_plans_refuse_it(dt):
    lib = L.lib()
    h = _plan(dt)
    try:
        assert lib.hiccl_reduce_plan_set_out_dtype(h, L.HICCL_FLOAT32) == 0, L.last_error()
        _refused(_add(lib, h, 0x100000, (0x200000,), 64, True), "plan_add_unscaled", "widened or accumulating plan")
        assert lib.hiccl_reduce_plan_set_accumulate(h, 1) == 0
        _refused(_add(lib, h, 0x100000, (0x200000,), 64, True), "plan_add_unscaled", "widened or accumulating plan")
        assert lib.hiccl_reduce_plan_num_unscaled(h) == 0 and lib.hiccl_reduce_plan_numcomp(h) == 0
        assert _add(lib, h, 0x100000, (0x200000,), 64, False) == 0, L.last_error()  # the plain add still works
    finally:
        lib.hiccl_reduce_plan_destroy(h)


@pytest.mark.parametrize("dt", (L.HICCL_FLOAT32, L.HICCL_BFLOAT16, L.HICCL_FLOAT8_E4M3))
def test_program_refuses_a_mixed_plan(dt):
    """hiccl_program_add_plan refuses any plan that has a scale, mixed or all
    unscaled; with the scale cleared the plan joins, flags and all."""
    lib = L.lib()
    h = _plan(dt)
    prog = ctypes.c_void_p()
    assert lib.hiccl_program_create(ctypes.byref(prog), dt, 0) == 0, L.last_error()
    try:
        assert lib.hiccl_reduce_plan_set_scale(h, ctypes.byref(ctypes.c_double(0.7))) == 0
        assert _add(lib, h, 0x100000, (0x200000, 0x300000), 100, True) == 0
        _refused(lib.hiccl_program_add_plan(prog, h), "program_add_plan", "scaled plan")  # every compute unscaled
        assert _add(lib, h, 0x400000, (0x500000, 0x600000), 100, False) == 0
        _refused(lib.hiccl_program_add_plan(prog, h), "program_add_plan", "scaled plan")  # mixed
        assert lib.hiccl_program_num_units(prog) == 0
        assert lib.hiccl_reduce_plan_set_scale(h, None) == 0
        assert lib.hiccl_program_add_plan(prog, h) == 0, L.last_error()
        assert lib.hiccl_program_num_units(prog) == 2
    finally:
        lib.hiccl_program_destroy(prog)
        lib.hiccl_reduce_plan_destroy(h)
