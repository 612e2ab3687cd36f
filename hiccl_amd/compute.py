"""Python mirror of the reference's reduction compute stage.

``reduce`` is one registered compute launched once (source/compute.h:90-91);
``Compute`` mirrors ``HiCCL::Compute<T>`` (source/compute.h:26-204):
``add`` / ``start`` / ``wait`` / ``report`` / ``measure`` with the same
argument meaning.  Both call straight into the HIP library through the C ABI
(include/hiccl_reduce.h); device memory and streams come from torch.
"""
import ctypes
import math
import numbers

import torch

from . import _lib as L


def _stream_handle(stream, device=None):
    if stream is None:
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


def _ptr_table(ptrs):
    t = (ctypes.c_void_p * max(1, len(ptrs)))()
    for k, p in enumerate(ptrs):
        t[k] = p
    return t


def _dtype_code(t):
    try:
        return L.DTYPE_OF_TORCH[t.dtype]
    except KeyError:
        raise TypeError(f"hiccl: unsupported dtype {t.dtype}") from None


_FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)  # OCP FP8: SUM (scaled too), MAX and MIN only


def _check_op(op, dtype):
    """torch.int64 stands for size_t under the sign-agnostic operators (SUM,
    PROD and the bitwise three: the same bits for either signedness); MAX and
    MIN on HICCL_UINT64 compare unsigned.  The bitwise operators take the
    integer types only."""
    if op in (L.HICCL_OP_MAX, L.HICCL_OP_MIN) and dtype == torch.int64:
        raise TypeError("hiccl: MAX / MIN on HICCL_UINT64 compare unsigned: pass torch.uint64, not torch.int64")
    if op in (L.HICCL_OP_BAND, L.HICCL_OP_BOR, L.HICCL_OP_BXOR) and dtype.is_floating_point:
        raise TypeError(f"hiccl: BAND / BOR / BXOR take the integer types only (int32, uint64), not {dtype}")
    if op == L.HICCL_OP_PROD and dtype in _FP8:
        raise TypeError(f"hiccl: PROD is not defined for the FP8 types, not {dtype}")


def _check_scale(scale, dtype, op=L.HICCL_OP_SUM):
    """A scaled sum (out = scale * sum, hiccl_reduce_scaled): floating types,
    SUM, a finite scale -- refused here, before any device work.  Returns the
    scale as a float."""
    if isinstance(dtype, torch.dtype):
        floating = dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16) + _FP8
    else:
        floating = int(dtype) in (L.HICCL_FLOAT32, L.HICCL_FLOAT64, L.HICCL_BFLOAT16, L.HICCL_FLOAT16,
                                  L.HICCL_FLOAT8_E4M3, L.HICCL_FLOAT8_E5M2)
    if not floating:
        raise TypeError(f"hiccl: scaled sums take the floating types only (f32, f64, bf16, f16, fp8), not {dtype}")
    if op != L.HICCL_OP_SUM:
        raise ValueError("hiccl: only sums are scaled: scale= goes with HICCL_OP_SUM")
    if isinstance(scale, torch.Tensor) and scale.ndim == 0 and not scale.is_complex():
        scale = scale.item()  # a 0-d tensor, as 1 / torch.tensor(n)
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real):  # numpy's real scalars are Real
        raise TypeError(f"hiccl: scale must be a real number, not {type(scale).__name__}")
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"hiccl: scale must be finite, not {scale}")
    return scale


def _check_tensor(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"hiccl: {what} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"hiccl: {what} must be a device tensor (the HIP path has no CPU mode)")
    if not t.is_contiguous():
        raise ValueError(f"hiccl: {what} must be contiguous")


def reduce(out, inputs, count=None, stream=None, config=None, op=L.HICCL_OP_SUM, scale=None):
    """out[:count] = ((0 + inputs[0]) + inputs[1]) + ... in the list order.

    ``scale`` (a finite number, floating dtypes, SUM only): the sum times
    ``scale``, multiplied once at store time (hiccl_reduce_scaled) -- an
    average is ``scale=1 / len(inputs)``.  f32 / f64: one IEEE multiply; bf16 /
    f16: an f32 multiply rounded to f32, then rounded to the type.

    ``op``: HICCL_OP_SUM (default), HICCL_OP_MAX, HICCL_OP_MIN, HICCL_OP_PROD
    or, on the integer types, HICCL_OP_BAND / _BOR / _BXOR -- the same fold
    from the operator's identity (IEEE 754-2019 maximum / minimum on the
    floating types: a NaN input gives NaN, -0 < +0; PROD: one multiply per
    input, rounded to the type, integers wrap; hiccl_reduce_op).

    Mirrors one compute of compute.h: inputs are summed in list order with
    the accumulator starting at 0 in the element type.  ``out`` may be one
    of the inputs (in place).  Asynchronous on ``stream`` (default: torch's
    current stream).  ``config``: dict of hiccl_reduce_config_t fields.
    """
    _check_tensor(out, "out")
    if count is None:
        count = out.numel()
    if count < 0:
        raise ValueError(f"hiccl: count={count} < 0")
    dt = _dtype_code(out)
    ptrs = []
    for k, x in enumerate(inputs):
        _check_tensor(x, f"inputs[{k}]")
        if x.device != out.device:
            raise ValueError(f"hiccl: inputs[{k}] is on {x.device}, out on {out.device}")
        if x.dtype != out.dtype:
            raise TypeError(f"hiccl: inputs[{k}] dtype {x.dtype} != out dtype {out.dtype}")
        if x.numel() < count:
            raise ValueError(f"hiccl: inputs[{k}] has {x.numel()} < count={count} elements")
        ptrs.append(x.data_ptr())
    if out.numel() < count:
        raise ValueError(f"hiccl: out has {out.numel()} < count={count} elements")
    _check_op(op, out.dtype)
    if scale is not None:
        scale = _check_scale(scale, out.dtype, op)
    tab = _ptr_table(ptrs)
    with torch.cuda.device(out.device):  # the library launches on the current device
        s = _stream_handle(stream, out.device)
        if scale is not None:
            cfg = ctypes.byref(L.ReduceConfig(**config)) if config is not None else None
            rc = L.lib().hiccl_reduce_scaled(dt, scale, ctypes.c_void_p(out.data_ptr()), tab, len(ptrs), count, s, cfg)
        elif op != L.HICCL_OP_SUM:
            cfg = ctypes.byref(L.ReduceConfig(**config)) if config is not None else None
            rc = L.lib().hiccl_reduce_op(dt, op, ctypes.c_void_p(out.data_ptr()), tab, len(ptrs), count, s, cfg)
        elif config is None:
            rc = L.lib().hiccl_reduce(dt, ctypes.c_void_p(out.data_ptr()), tab, len(ptrs), count, s)
        else:
            cfg = L.ReduceConfig(**config)
            rc = L.lib().hiccl_reduce_ex(dt, ctypes.c_void_p(out.data_ptr()), tab, len(ptrs), count, s,
                                         ctypes.byref(cfg))
    L.check(rc, "hiccl_reduce")
    return out


def reduce_ptrs(dtype_code, out_ptr, in_ptrs, count, stream=None, config=None, op=L.HICCL_OP_SUM, scale=None):
    """Raw-pointer form (pointers already offset), used by the Comm layer."""
    if scale is not None:
        scale = _check_scale(scale, dtype_code, op)
    tab = _ptr_table(list(in_ptrs))
    s = _stream_handle(stream)
    if scale is not None:
        cfg = ctypes.byref(L.ReduceConfig(**config)) if config is not None else None
        rc = L.lib().hiccl_reduce_scaled(dtype_code, scale, ctypes.c_void_p(out_ptr), tab, len(in_ptrs), count, s, cfg)
    elif op != L.HICCL_OP_SUM:
        cfg = ctypes.byref(L.ReduceConfig(**config)) if config is not None else None
        rc = L.lib().hiccl_reduce_op(dtype_code, op, ctypes.c_void_p(out_ptr), tab, len(in_ptrs), count, s, cfg)
    elif config is None:
        rc = L.lib().hiccl_reduce(dtype_code, ctypes.c_void_p(out_ptr), tab, len(in_ptrs), count, s)
    else:
        cfg = L.ReduceConfig(**config)
        rc = L.lib().hiccl_reduce_ex(dtype_code, ctypes.c_void_p(out_ptr), tab, len(in_ptrs), count, s,
                                     ctypes.byref(cfg))
    L.check(rc, "hiccl_reduce")


_WIDEN_IN = (torch.bfloat16, torch.float16) + _FP8  # inputs of a widened sum; its output is f32


def _check_widened(in_dtype, out_dtype):
    """The dtypes of a widened sum (hiccl_reduce_widened): bf16, f16 or FP8
    inputs, an f32 output -- refused here, before any device work.  Torch
    dtypes or HICCL_* codes."""
    out_ok = out_dtype == torch.float32 if isinstance(out_dtype, torch.dtype) else int(out_dtype) == L.HICCL_FLOAT32
    if not out_ok:
        raise TypeError(f"hiccl: a widened sum writes torch.float32, not {out_dtype}")
    if isinstance(in_dtype, torch.dtype):
        in_ok = in_dtype in _WIDEN_IN
    else:
        in_ok = int(in_dtype) in (L.HICCL_BFLOAT16, L.HICCL_FLOAT16, L.HICCL_FLOAT8_E4M3, L.HICCL_FLOAT8_E5M2)
    if not in_ok:
        raise TypeError(f"hiccl: widened sums take bf16, f16, float8_e4m3fn or float8_e5m2 inputs, not {in_dtype}")


def _check_widened_config(config):
    if config is not None and config.get("acc", L.HICCL_ACC_NATIVE) != L.HICCL_ACC_NATIVE:
        raise ValueError("hiccl: a widened sum always accumulates in f32: leave acc at HICCL_ACC_NATIVE")


def _check_accumulate(accumulate, widened=True):
    """``accumulate=`` is a bool, and goes with a widened sum only."""
    if not isinstance(accumulate, bool):
        raise TypeError(f"hiccl: accumulate must be a bool, not {type(accumulate).__name__}")
    if accumulate and not widened:
        raise ValueError("hiccl: only a widened sum accumulates: accumulate=True goes with out_dtype=torch.float32 "
                         "(a same-type sum accumulates by passing out as input 0)")


def _check_weights(weights, n, out, out_ptr=None, count=None):
    """The weights of a weighted sum: a contiguous float32 tensor of ``n``
    elements on the output's device that does not overlap the output -- refused
    here, before any device work.  A Python sequence is not taken: the caller
    makes the tensor, so nothing is uploaded behind their back.  Returns the
    tensor's address."""
    if not isinstance(weights, torch.Tensor):
        raise TypeError(f"hiccl: weights must be a torch.float32 tensor on the device, not {type(weights).__name__} "
                        "(the kernels read the weights from device memory when they run)")
    if weights.dtype != torch.float32:
        raise TypeError(f"hiccl: weights must be torch.float32, not {weights.dtype}")
    if not weights.is_cuda:
        raise ValueError("hiccl: weights must live in device memory (the kernels read them when they run)")
    if out is not None and weights.device != out.device:
        raise ValueError(f"hiccl: weights are on {weights.device}, out on {out.device}")
    if not weights.is_contiguous():
        raise ValueError("hiccl: weights must be contiguous")
    if weights.numel() != n:
        raise ValueError(f"hiccl: {weights.numel()} weights for {n} inputs")
    w0 = weights.data_ptr()
    if out_ptr is not None and count and n and w0 < out_ptr + 4 * count and out_ptr < w0 + 4 * n:
        raise ValueError("hiccl: the weights overlap the output")
    return w0


def reduce_widened(out, inputs, count=None, stream=None, config=None, scale=None, accumulate=False, weights=None):
    """out[:count] = ((0.0f + float(inputs[0])) + float(inputs[1])) + ... in the
    list order, every add an f32 add: bf16, f16 or FP8 ``inputs`` (one dtype)
    summed into a ``torch.float32`` ``out`` in one pass (hiccl_reduce_widened)
    -- low-precision gradient buckets into f32 master gradients.  The result is
    :func:`reduce` in f32 on ``x.float()`` inputs, bit for bit, without the
    converted copies.

    ``scale``: the f32 sum times ``float32(scale)``, one f32 multiply at store
    time.  ``out`` must not overlap any input (the element sizes differ, so
    nothing runs in place).  Asynchronous on ``stream``; ``config`` as
    :func:`reduce`'s, ``acc`` left native.  The kernels are untuned: a config
    that names a shape they lack raises HicclError.

    ``accumulate=True``: ``out += scale * sum`` (hiccl_reduce_accumulate) --
    the sum is finished first, scaled, then added to ``out`` as it was: three
    separately rounded f32 operations.  Every call adds once more.

    ``weights``: a contiguous ``torch.float32`` tensor of ``len(inputs)``
    elements on ``out``'s device; input k then counts as
    ``fl32(weights[k] * float(inputs[k]))`` (hiccl_reduce_weighted: a multiply
    and an add, separately rounded -- the words of ``reduce`` on the f32 copies
    ``x.float() * w``).  The kernel reads the weights when it runs: a kernel
    that wrote them earlier on the same stream is seen, nothing synchronises,
    and a captured graph replays with the values the tensor then holds.  They
    are not validated and must not overlap ``out``.
    """
    _check_tensor(out, "out")
    if count is None:
        count = out.numel()
    if count < 0:
        raise ValueError(f"hiccl: count={count} < 0")
    inputs = list(inputs)
    in_dtype = None
    ptrs = []
    for k, x in enumerate(inputs):
        _check_tensor(x, f"inputs[{k}]")
        if x.device != out.device:
            raise ValueError(f"hiccl: inputs[{k}] is on {x.device}, out on {out.device}")
        if in_dtype is None:
            in_dtype = x.dtype
        elif x.dtype != in_dtype:
            raise TypeError(f"hiccl: inputs[{k}] dtype {x.dtype} != inputs[0] dtype {in_dtype}")
        if x.numel() < count:
            raise ValueError(f"hiccl: inputs[{k}] has {x.numel()} < count={count} elements")
        ptrs.append(x.data_ptr())
    if in_dtype is None:
        raise ValueError("hiccl: reduce_widened needs at least one input to tell the input dtype "
                         "(reduce_widened_ptrs takes it as an argument)")
    _check_widened(in_dtype, out.dtype)
    if out.numel() < count:
        raise ValueError(f"hiccl: out has {out.numel()} < count={count} elements")
    if weights is not None:
        _check_weights(weights, len(ptrs), out, out.data_ptr(), count)
    with torch.cuda.device(out.device):  # the library launches on the current device
        reduce_widened_ptrs(L.DTYPE_OF_TORCH[in_dtype], out.data_ptr(), ptrs, count,
                            stream=_stream_handle(stream, out.device).value or 0, config=config, scale=scale,
                            accumulate=accumulate, weights=weights)
    return out


def reduce_widened_ptrs(in_dtype_code, out_ptr, in_ptrs, count, stream=None, config=None, scale=None,
                        out_dtype_code=L.HICCL_FLOAT32, accumulate=False, weights=None):
    """Raw-pointer form of :func:`reduce_widened` (pointers already offset);
    ``weights`` is a tensor here too."""
    _check_accumulate(accumulate)
    _check_widened(in_dtype_code, out_dtype_code)
    _check_widened_config(config)
    alpha = None
    if scale is not None:
        alpha = ctypes.byref(ctypes.c_double(_check_scale(scale, in_dtype_code)))
    tab = _ptr_table(list(in_ptrs))
    cfg = ctypes.byref(L.ReduceConfig(**config)) if config is not None else None
    if weights is not None:
        w0 = _check_weights(weights, len(in_ptrs), None, out_ptr, count)
        rc = L.lib().hiccl_reduce_weighted(int(in_dtype_code), int(out_dtype_code), alpha, 1 if accumulate else 0,
                                           ctypes.c_void_p(out_ptr), tab, ctypes.c_void_p(w0), len(in_ptrs), count,
                                           _stream_handle(stream), cfg)
        L.check(rc, "hiccl_reduce_weighted")
        return
    fn = L.lib().hiccl_reduce_accumulate if accumulate else L.lib().hiccl_reduce_widened
    rc = fn(int(in_dtype_code), int(out_dtype_code), alpha, ctypes.c_void_p(out_ptr), tab, len(in_ptrs), count,
            _stream_handle(stream), cfg)
    L.check(rc, "hiccl_reduce_accumulate" if accumulate else "hiccl_reduce_widened")


def bucket(n, count, dtype=torch.float32, device=None):
    """A reduction bucket in the library's layout (hiccl_bucket_alloc): n
    inputs and one output of ``count`` elements carved from ONE device
    allocation, buffer j at j x hiccl_bucket_stride (the buffer rounded up to
    64 KiB, plus 64 KiB), so the n + 1 streams keep one fixed relative
    placement.  The slab comes from torch's allocator
    (one hipMalloc for a fresh large block) and lives as long as any view.
    Returns (inputs, output): contiguous 1-D views."""
    esz = torch.empty((), dtype=dtype).element_size()
    stride = L.lib().hiccl_bucket_stride(L.DTYPE_OF_TORCH.get(dtype, -1), count)
    if not stride:
        raise ValueError(f"hiccl: no bucket layout for dtype {dtype}, count {count}")
    assert stride % esz == 0
    se = stride // esz
    slab = torch.empty((n + 1) * se, dtype=dtype, device=device if device is not None else "cuda")
    views = [slab[j * se:j * se + count] for j in range(n + 1)]
    return views[:n], views[n]


def auto_choice(dtype, count, n, config=None, cus=256, op=L.HICCL_OP_SUM, scale=False, out_dtype=None,
                accumulate=False, weighted=False):
    """What a one-shot call (and a one-compute plan at TILE unroll 2 / 4 or
    AUTO) resolves to on a GPU of ``cus`` CUs, without a device:
    ``hiccl_reduce_auto_choice_ex`` (``op`` other than SUM:
    ``hiccl_reduce_auto_choice_op``; ``scale=True``, a scaled sum:
    ``hiccl_reduce_auto_choice_scaled``).  ``dtype``: a torch dtype or an
    HICCL_* code; ``n`` may be a plan's packet-weighted mean.  Returns a dict
    with engine, unroll, blocks_per_cu, dynamic and store_policy (2 nt, 4
    write-through); raises HicclError for a config no kernel has.
    ``out_dtype`` (torch.float32 with a bf16, f16 or FP8 ``dtype``): a widened
    sum, ``hiccl_reduce_auto_choice_widened`` -- the same answer scaled or not;
    with ``accumulate=True`` ``hiccl_reduce_auto_choice_accumulate``, the same
    answer again.  ``weighted=True`` (with ``out_dtype``):
    ``hiccl_reduce_auto_choice_weighted``, which answers what the unweighted
    entry of the same ``accumulate`` answers."""
    _check_accumulate(accumulate, out_dtype is not None)
    if weighted and out_dtype is None:
        raise ValueError("hiccl: only a widened sum is weighted: weighted=True goes with out_dtype=torch.float32")
    dt = L.DTYPE_OF_TORCH[dtype] if isinstance(dtype, torch.dtype) else int(dtype)
    cfg = ctypes.byref(L.ReduceConfig(**config)) if config else None
    out = [ctypes.c_int() for _ in range(5)]
    if out_dtype is not None:
        _check_widened(dtype if isinstance(dtype, torch.dtype) else dt, out_dtype)
        if op != L.HICCL_OP_SUM:
            raise ValueError("hiccl: only sums are widened: out_dtype= goes with HICCL_OP_SUM")
        _check_widened_config(config)
        if weighted:
            rc = L.lib().hiccl_reduce_auto_choice_weighted(dt, 1 if accumulate else 0, cfg, count, float(n), cus,
                                                           *[ctypes.byref(v) for v in out])
        else:
            fn = (L.lib().hiccl_reduce_auto_choice_accumulate if accumulate
                  else L.lib().hiccl_reduce_auto_choice_widened)
            rc = fn(dt, cfg, count, float(n), cus, *[ctypes.byref(v) for v in out])
    elif scale:
        _check_scale(1.0, dtype if isinstance(dtype, torch.dtype) else dt, op)
        rc = L.lib().hiccl_reduce_auto_choice_scaled(dt, cfg, count, float(n), cus, *[ctypes.byref(v) for v in out])
    elif op != L.HICCL_OP_SUM:
        rc = L.lib().hiccl_reduce_auto_choice_op(dt, op, cfg, count, float(n), cus, *[ctypes.byref(v) for v in out])
    else:
        rc = L.lib().hiccl_reduce_auto_choice_ex(dt, cfg, count, float(n), cus, *[ctypes.byref(v) for v in out])
    L.check(rc, "hiccl_reduce_auto_choice")
    return dict(zip(("engine", "unroll", "blocks_per_cu", "dynamic", "store_policy"), (v.value for v in out)))


class Compute:
    """``HiCCL::Compute<T>`` (source/compute.h:26-204) on the batched plan.

    add(inputbuf, outputbuf, count, compid)  compute.h:47-85 -- records the
        compute only when ``myid == compid`` (SPMD: every rank calls add).
        ``inputbuf`` is a list of tensors or (tensor, element_offset) pairs,
        ``outputbuf`` a tensor or (tensor, element_offset).  ``count == 0``
        is checked and recorded nowhere, as the C plan does: ``numcomp`` is
        hiccl_reduce_plan_numcomp.
    start()   compute.h:87-106 -- ONE batched kernel for all computes.
    wait()    compute.h:107-117.
    report()  compute.h:119-135 (local numbers; the Comm layer gathers).
    measure(warmup, numiter[, count])  compute.h:137-203.
    """

    def __init__(self, dtype=torch.float32, device=None, myid=0, acc=L.HICCL_ACC_NATIVE,
                 engine=L.HICCL_ENGINE_AUTO, config=None, op=L.HICCL_OP_SUM, scale=None, out_dtype=None,
                 accumulate=False, weighted=False):
        _check_accumulate(accumulate, out_dtype is not None)
        if weighted and out_dtype is None:
            raise ValueError("hiccl: only a widened plan is weighted: weighted=True goes with out_dtype=torch.float32")
        self.dtype = dtype
        self.code = L.DTYPE_OF_TORCH[dtype]
        if scale is not None:
            scale = _check_scale(scale, dtype, op)
        # a widened plan (hiccl_reduce_plan_set_out_dtype): `dtype` inputs, f32 outputs
        self.out_dtype = dtype if out_dtype is None else out_dtype
        if out_dtype is not None:
            _check_widened(dtype, out_dtype)
            if op != L.HICCL_OP_SUM:
                raise ValueError("hiccl: only sums are widened: out_dtype= goes with HICCL_OP_SUM")
            if acc != L.HICCL_ACC_NATIVE:
                raise ValueError("hiccl: a widened sum always accumulates in f32: leave acc at HICCL_ACC_NATIVE")
            _check_widened_config(config)
        if device is None:
            device = torch.cuda.current_device()
        self.device = device
        self.myid = myid
        self.numcomp = 0
        self.inputbuf = []
        self.outputbuf = []
        self.count = []
        self._keep = []  # keep tensors alive while registered
        h = ctypes.c_void_p()
        L.check(L.lib().hiccl_reduce_plan_create(ctypes.byref(h), self.code, device), "plan_create")
        self._plan = h
        if acc != L.HICCL_ACC_NATIVE:
            L.check(L.lib().hiccl_reduce_plan_set_acc(self._plan, acc), "plan_set_acc")
        if engine != L.HICCL_ENGINE_AUTO:
            L.check(L.lib().hiccl_reduce_plan_set_engine(self._plan, engine), "plan_set_engine")
        if config is not None:
            self.set_config(config)
        if op != L.HICCL_OP_SUM:
            self.set_op(op)
        if out_dtype is not None:
            L.check(L.lib().hiccl_reduce_plan_set_out_dtype(self._plan, L.DTYPE_OF_TORCH[out_dtype]),
                    "plan_set_out_dtype")
        if weighted:  # before the first add, as the output dtype
            L.check(L.lib().hiccl_reduce_plan_set_weighted(self._plan, 1), "plan_set_weighted")
        if scale is not None:
            self.set_scale(scale)
        if accumulate:
            self.set_accumulate(True)

    def weighted(self):
        """Is the plan weighted (hiccl_reduce_plan_weighted: ``weighted=True``
        at construction)?  Every add then brings ``weights=``."""
        return L.lib().hiccl_reduce_plan_weighted(self._plan) == 1

    def set_accumulate(self, on):
        """Accumulation of a widened plan (hiccl_reduce_plan_set_accumulate):
        every compute writes ``out + scale * sum`` from the next launch on
        (``start(each=True)`` too), and every launch adds once more; ``False``
        goes back to overwriting.  At any time, like :meth:`set_scale`.  A
        widened plan only, and never with HICCL_PEER_STORES."""
        _check_accumulate(on, self.out_dtype != self.dtype)
        if on and self.peer() & L.HICCL_PEER_STORES:
            raise ValueError("hiccl: an accumulating plan takes no HICCL_PEER_STORES (the old output is read where it "
                             "is written: keep it in local memory)")
        L.check(L.lib().hiccl_reduce_plan_set_accumulate(self._plan, 1 if on else 0), "plan_set_accumulate")

    def accumulate(self):
        """Does the plan accumulate (hiccl_reduce_plan_accumulate)?"""
        return L.lib().hiccl_reduce_plan_accumulate(self._plan) == 1

    def set_scale(self, scale):
        """Scale of the plan's sums (hiccl_reduce_plan_set_scale): every
        compute writes ``scale`` times its sum from the next launch on
        (``start(each=True)`` too); ``None`` clears it.  At any time, like
        :meth:`set_acc`.  Floating dtypes and SUM only; a program takes no
        scaled plan."""
        if scale is None:
            L.check(L.lib().hiccl_reduce_plan_set_scale(self._plan, None), "plan_set_scale")
            return
        a = ctypes.c_double(_check_scale(scale, self.dtype, self.op()))
        L.check(L.lib().hiccl_reduce_plan_set_scale(self._plan, ctypes.byref(a)), "plan_set_scale")

    def scale(self):
        """The plan's scale, or None (hiccl_reduce_plan_scale)."""
        a = ctypes.c_double()
        return a.value if L.lib().hiccl_reduce_plan_scale(self._plan, ctypes.byref(a)) == 1 else None

    def set_op(self, op):
        """Operator of the plan's launches (hiccl_reduce_plan_set_op:
        HICCL_OP_SUM / _MAX / _MIN / _PROD / _BAND / _BOR / _BXOR), at any
        time; the next launch re-uploads."""
        _check_op(op, self.dtype)
        L.check(L.lib().hiccl_reduce_plan_set_op(self._plan, op), "plan_set_op")

    def op(self):
        return L.lib().hiccl_reduce_plan_op(self._plan)

    def set_config(self, config):
        """Kernel configuration of the plan (dict of hiccl_reduce_config_t
        fields; hiccl_reduce_plan_set_config).  A field the plan kernels do
        not honour raises HicclError."""
        cfg = L.ReduceConfig(**config)
        L.check(L.lib().hiccl_reduce_plan_set_config(self._plan, ctypes.byref(cfg)), "plan_set_config")

    def set_engine(self, engine):
        """Engine of the plan's launches (hiccl_reduce_plan_set_engine); the
        rest of the configuration stays."""
        L.check(L.lib().hiccl_reduce_plan_set_engine(self._plan, engine), "plan_set_engine")

    def set_acc(self, acc):
        """Accumulation mode (hiccl_reduce_plan_set_acc); the rest of the
        configuration stays."""
        L.check(L.lib().hiccl_reduce_plan_set_acc(self._plan, acc), "plan_set_acc")

    def set_peer(self, flags):
        """Peer-memory policy of the plan's launches (hiccl_reduce_plan_set_peer):
        HICCL_PEER_STORES (outputs in another GPU's memory: system-scope
        write-through stores) | HICCL_PEER_LOADS (inputs there: system-scope
        loads).  Same results.  An accumulating plan takes HICCL_PEER_LOADS only."""
        if flags & L.HICCL_PEER_STORES and self.accumulate():
            raise ValueError("hiccl: an accumulating plan takes no HICCL_PEER_STORES (the old output is read where it "
                             "is written: keep it in local memory)")
        L.check(L.lib().hiccl_reduce_plan_set_peer(self._plan, flags), "plan_set_peer")

    def peer(self):
        return L.lib().hiccl_reduce_plan_peer(self._plan)

    def store_policy(self):
        """The store form of the plan's launches (hiccl_reduce_plan_store_policy):
        2 nt, 4 system-scope write-through."""
        return L.lib().hiccl_reduce_plan_store_policy(self._plan)

    def engine(self):
        """Engine the last upload resolved to (HICCL_ENGINE_TILE / _PHASE)."""
        return L.lib().hiccl_reduce_plan_engine(self._plan)

    @staticmethod
    def _ptr(buf, esz):
        if isinstance(buf, tuple):
            t, off = buf
        else:
            t, off = buf, 0
        return t, t.data_ptr() + off * esz

    def add(self, inputbuf, outputbuf, count, compid, unscaled=False, weights=None):
        """Register one compute on its owning rank.  ``unscaled``: in a plan
        that has a scale this compute writes the plain sum
        (hiccl_reduce_plan_add_unscaled: an intermediate compute of a
        hierarchical average); without a scale it changes nothing.  A widened
        or accumulating plan takes none.  ``weights``: on a weighted plan
        (``weighted=True``) the compute's f32 weights, one per input, a
        contiguous float32 tensor on the plan's device
        (hiccl_reduce_plan_add_weighted); the plan keeps the tensor and every
        launch reads the values it then holds."""
        if self.myid != compid:
            return
        if weights is None and self.weighted():
            raise ValueError("hiccl: a weighted plan takes weighted computes only: add(..., weights=tensor)")
        if weights is not None and not self.weighted():
            raise ValueError("hiccl: the plan is not weighted: Compute(..., out_dtype=torch.float32, weighted=True)")
        if unscaled and self.out_dtype != self.dtype:
            raise ValueError("hiccl: a widened or accumulating plan takes no unscaled compute (one scale per plan)")
        esz = L.lib().hiccl_dtype_size(self.code)
        ins = [self._ptr(b, esz) for b in inputbuf]
        ot, op = self._ptr(outputbuf, L.lib().hiccl_dtype_size(L.DTYPE_OF_TORCH[self.out_dtype]))
        tab = _ptr_table([p for _, p in ins])
        if weights is not None:
            w0 = _check_weights(weights, len(ins), ot, op, count)
            L.check(L.lib().hiccl_reduce_plan_add_weighted(self._plan, ctypes.c_void_p(op), tab, ctypes.c_void_p(w0),
                                                           len(ins), count), "plan_add_weighted")
        else:
            fn = L.lib().hiccl_reduce_plan_add_unscaled if unscaled else L.lib().hiccl_reduce_plan_add
            L.check(fn(self._plan, ctypes.c_void_p(op), tab, len(ins), count),
                    "plan_add_unscaled" if unscaled else "plan_add")
        if count == 0:  # validated, then dropped by the plan (a no-op): numcomp is hiccl_reduce_plan_numcomp
            return
        self._keep.append((ot, [t for t, _ in ins], weights))
        self.inputbuf.append([p for _, p in ins])
        self.outputbuf.append(op)
        self.count.append(count)
        self.numcomp += 1

    def num_unscaled(self):
        """Computes added with ``unscaled=True`` (hiccl_reduce_plan_num_unscaled)."""
        return L.lib().hiccl_reduce_plan_num_unscaled(self._plan)

    def stream_handle(self):
        """The plan's own stream (hipStream_t as int)."""
        return L.lib().hiccl_reduce_plan_stream(self._plan)

    def start(self, stream=None, each=False):
        """Launch on ``stream`` (torch stream or raw handle); default = the
        plan's own stream (the reference keeps one per compute, compute.h:76-78),
        ordered after the work already queued on torch's current stream (the
        inputs it produced), so no synchronisation is needed first."""
        if stream is None:
            own = torch.cuda.ExternalStream(self.stream_handle(), device=self.device)
            own.wait_stream(torch.cuda.current_stream(self.device))
            s = ctypes.c_void_p(self.stream_handle())
        else:
            s = _stream_handle(stream, self.device)
        fn = L.lib().hiccl_reduce_plan_launch_each if each else L.lib().hiccl_reduce_plan_launch
        L.check(fn(self._plan, s), "plan_launch")

    def enqueue(self, stream=None):
        """Launch on ``stream`` (default torch's current stream) without
        remembering it for :meth:`wait` (hiccl_reduce_plan_enqueue): for
        stream-ordered pipelines that synchronise the stream themselves."""
        L.check(L.lib().hiccl_reduce_plan_enqueue(self._plan, _stream_handle(stream, self.device)), "plan_enqueue")

    def wait(self):
        L.check(L.lib().hiccl_reduce_plan_sync(self._plan), "plan_sync")

    def bytes(self):
        """Sum of count * (n + 1) * sizeof(T) (compute.h:197-203); a widened
        plan: count * (n * sizeof(T) + 4), an accumulating one + 8."""
        return L.lib().hiccl_reduce_plan_bytes(self._plan)

    def report(self):
        numinput = sum(len(x) for x in self.inputbuf)
        return f"numcomp: {self.numcomp}({numinput})"

    def measure(self, warmup, numiter, count=None, each=False):
        """Time start()+wait() like compute.h:137-196; returns the stats dict.

        ``count`` is the element count the GB/s figure is priced on
        (compute.h:188); default = the two-argument overload's
        sum of count*(n+1) (compute.h:197-203), i.e. reads + writes.
        """
        import time
        data = (self.bytes() if count is None else count * torch.tensor([], dtype=self.dtype).element_size())
        times = []
        for it in range(-warmup, numiter):
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            self.start(each=each)
            self.wait()
            t = time.perf_counter() - t0
            if it >= 0:
                times.append(t)
        times.sort()
        avg = sum(times) / len(times)
        stats = {"min": times[0], "median": times[len(times) // 2], "max": times[-1], "avg": avg,
                 "data": data}
        for k in ("min", "median", "max", "avg"):
            stats[k + "_GBps"] = data / stats[k] / 1e9
        return stats

    def close(self):
        if self._plan:
            L.lib().hiccl_reduce_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Program:
    """A program (include/hiccl_reduce.h ``hiccl_program_*``): signal/wait
    phases folded into the launch of one batch of independent computes --
    the phases run first (one wave, in order), the units after the last
    phase.  HiCCL::Comm records its stream-ordered pipeline as programs.

    add_signal(sig_ptrs, wait_ptrs)   one phase (device flag addresses),
                                      before the first add_plan.
    add_plan(compute)                 the computes a :class:`Compute` holds
                                      now (its dtype must be the program's,
                                      or torch.uint8 = exact byte copies).
    launch(epochs, epoch_dev, err, timeout_s, stream)
    """

    def __init__(self, dtype=torch.float32, device=None):
        if device is None:
            device = torch.cuda.current_device()
        self.device = device
        h = ctypes.c_void_p()
        L.check(L.lib().hiccl_program_create(ctypes.byref(h), L.DTYPE_OF_TORCH[dtype], device), "program_create")
        self._prog = h
        self._keep = []

    def add_signal(self, sig_ptrs, wait_ptrs):
        st, wt = _ptr_table(list(sig_ptrs)), _ptr_table(list(wait_ptrs))
        L.check(L.lib().hiccl_program_add_signal(self._prog, st, len(sig_ptrs), wt, len(wait_ptrs)),
                "program_add_signal")

    def add_plan(self, compute):
        L.check(L.lib().hiccl_program_add_plan(self._prog, compute._plan), "program_add_plan")
        self._keep.append(compute)

    def set_max_workgroups(self, n):
        """Cap the launch at ``n`` workgroups (0: the default)."""
        L.check(L.lib().hiccl_program_set_max_workgroups(self._prog, int(n)), "program_set_max_workgroups")

    def units(self):
        return L.lib().hiccl_program_num_units(self._prog)

    def phases(self):
        return L.lib().hiccl_program_num_phases(self._prog)

    def launch(self, epochs=(), epoch_dev=None, err=None, timeout_s=10.0, stream=None):
        ep = (ctypes.c_uint32 * max(1, len(epochs)))(*epochs)
        L.check(L.lib().hiccl_program_launch(self._prog, ep, ctypes.c_void_p(epoch_dev or 0),
                                             ctypes.c_void_p(err or 0), float(timeout_s),
                                             _stream_handle(stream, self.device)), "program_launch")

    def close(self):
        if self._prog:
            L.lib().hiccl_program_destroy(self._prog)
            self._prog = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostPipe:
    """Host-resident buckets (include/hiccl_reduce.h hiccl_host_pipe_*):
    ``reduce(out, inputs)`` sums host tensors in list order on the GPU,
    staging ``chunk_bytes`` per input through device memory with H2D /
    kernel / D2H pipelined over ``depth`` streams.  Blocking; same bits as
    :func:`reduce`.  Pin the tensors (``pin_memory()``) for the overlap.
    ``op``: the operator (hiccl_host_pipe_set_op), default SUM.  ``scale``:
    a scaled sum (hiccl_host_pipe_set_scale), as :func:`reduce`'s."""

    def __init__(self, dtype=torch.float32, device=None, chunk_bytes=0, depth=0, op=L.HICCL_OP_SUM, scale=None):
        self.dtype = dtype
        self.code = L.DTYPE_OF_TORCH[dtype]
        self._op = op
        if scale is not None:
            scale = _check_scale(scale, dtype, op)
        if device is None:
            device = torch.cuda.current_device()
        h = ctypes.c_void_p()
        L.check(L.lib().hiccl_host_pipe_create(ctypes.byref(h), self.code, device, chunk_bytes, depth),
                "host_pipe_create")
        self._pipe = h
        if op != L.HICCL_OP_SUM:
            _check_op(op, dtype)
            L.check(L.lib().hiccl_host_pipe_set_op(self._pipe, op), "host_pipe_set_op")
        if scale is not None:
            self.set_scale(scale)

    def set_scale(self, scale):
        """Scale of the pipe's sums from the next reduce on; ``None`` clears it."""
        if scale is None:
            L.check(L.lib().hiccl_host_pipe_set_scale(self._pipe, None), "host_pipe_set_scale")
            return
        a = ctypes.c_double(_check_scale(scale, self.dtype, self._op))
        L.check(L.lib().hiccl_host_pipe_set_scale(self._pipe, ctypes.byref(a)), "host_pipe_set_scale")

    def reduce(self, out, inputs, count=None):
        for k, t in enumerate([out] + list(inputs)):
            what = "out" if k == 0 else f"inputs[{k - 1}]"
            if not isinstance(t, torch.Tensor) or t.is_cuda:
                raise ValueError(f"hiccl: {what} must be a host tensor (HostPipe stages it to the GPU)")
            if not t.is_contiguous():
                raise ValueError(f"hiccl: {what} must be contiguous")
            if t.dtype != self.dtype:
                raise TypeError(f"hiccl: {what} dtype {t.dtype} != pipe dtype {self.dtype}")
        if count is None:
            count = out.numel()
        if any(t.numel() < count for t in [out] + list(inputs)):
            raise ValueError(f"hiccl: a buffer has fewer than count={count} elements")
        tab = _ptr_table([t.data_ptr() for t in inputs])
        L.check(L.lib().hiccl_host_pipe_reduce(self._pipe, ctypes.c_void_p(out.data_ptr()), tab,
                                               len(inputs), count), "host_pipe_reduce")
        return out

    def close(self):
        if self._pipe:
            L.lib().hiccl_host_pipe_destroy(self._pipe)
            self._pipe = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_uniform(t, seed, k, first=0, stream=None):
    """Synthetic input k: uniform [-1,1) of hash(seed, k, first + i) (matches the oracle)."""
    _check_tensor(t, "t")
    L.check(L.lib().hiccl_fill_uniform(_dtype_code(t), ctypes.c_void_p(t.data_ptr()), t.numel(),
                                       seed, k, first, _stream_handle(stream)), "fill_uniform")
    return t


def stream_copy(dst, src, nbytes=None, stream=None):
    """Plain 16-B/lane device copy (the achievable-bandwidth ceiling)."""
    if nbytes is None:
        nbytes = src.numel() * src.element_size()
    L.check(L.lib().hiccl_stream_copy(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                      nbytes, _stream_handle(stream)), "stream_copy")
