"""CPU tier: the hostile inputs (tests/hostile.py) and the reference.

tests/test_hostile_gpu.py compares every kernel with ``oracle.reduce`` on
hostile inputs.  This file shows, without a GPU, that the comparison means
what it should: every class really occurs, the arrays are deterministic, the
oracle equals an independent NumPy restatement of the in-order sum on them
(and the reference's own reduce_kernel where oracle/_ref was built), and NaN
outputs -- which bits_equal compares by NaN-ness only -- stay a minority
while Inf, zero and subnormal outputs all occur.
"""
import ctypes
import os

import numpy as np
import pytest

import hostile as H
from conftest import REF_SO, bits_equal, first_mismatch

NS = [1, 2, 3, 8, 9, 17]
KINDS = ["f32", "f64", "bf16"]
COUNT = 17 * 241 + 5  # every class 241 or 242 times, on every residue mod 2, 4 and 8
REF16_SO = os.path.join(os.path.dirname(REF_SO), "libhiccl_ref_bf16.so")


def _bf16_round(f):
    """f32 -> bf16 bits, round to nearest even, stated on the dropped half:
    more than half an ulp rounds up, exactly half rounds to the even
    neighbour (a carry out of the largest finite value gives Inf); NaN stays
    NaN."""
    u = np.asarray(f, np.float32).view(np.uint32)
    keep, drop = (u >> 16).astype(np.uint32), u & 0xFFFF
    up = (drop > 0x8000) | ((drop == 0x8000) & ((keep & 1) == 1))
    r = (keep + up).astype(np.uint16)
    nan = np.isnan(f)
    r[nan] = 0x7FC0
    return r


def numpy_in_order(kind, x, wide=False):
    """T acc = 0; for k: acc += in[k][i], restated with NumPy arrays."""
    with np.errstate(all="ignore"):
        if kind != "bf16":
            acc = np.zeros(x.shape[1], x.dtype)
            for k in range(x.shape[0]):
                acc = (acc + x[k]).astype(x.dtype)
            return acc
        xf = H.bf16_to_f32(x)
        if wide:  # f32 accumulator, one rounding at the end
            acc = np.zeros(x.shape[1], np.float32)
            for k in range(x.shape[0]):
                acc = (acc + xf[k]).astype(np.float32)
            return _bf16_round(acc)
        acc = np.zeros(x.shape[1], np.uint16)
        for k in range(x.shape[0]):
            acc = _bf16_round((H.bf16_to_f32(acc) + xf[k]).astype(np.float32))
        return acc


def _reference(kind):
    """The reference's own reduce_kernel<T> (oracle/_ref), or None."""
    path, fn = {"f32": (REF_SO, "ref_reduce_f32"), "f64": (REF_SO, "ref_reduce_f64"),
                "bf16": (REF16_SO, "ref_reduce_bf16")}[kind]
    if not os.path.exists(path):
        return None
    f = getattr(ctypes.CDLL(path), fn)
    f.restype = None

    def run(x):
        out = np.empty(x.shape[1], x.dtype)
        rows = [np.ascontiguousarray(r) for r in x]
        tab = (ctypes.c_void_p * max(1, len(rows)))(*[r.ctypes.data for r in rows])
        f(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(x.shape[1]), tab, ctypes.c_int(len(rows)))
        return out
    return run


def _dtype(kind):
    return H.KINDS[kind]["dtype"]


def _arrays(kind, n):
    return [H.hostile(kind, n, COUNT, shift=s, seed=n) for s in (0, 5, 11)] + \
           [H.raw_bits(kind, n, COUNT, seed=n), H.raw_bits(kind, n, COUNT, seed=n, near=True)]


@pytest.mark.parametrize("kind", KINDS)
def test_every_class_occurs_and_is_what_it_says(kind):
    n = 9
    x = H.hostile(kind, n, COUNT, shift=3, seed=1)
    assert x.shape == (n, COUNT) and x.dtype == _dtype(kind)
    cls = H.class_of(COUNT, 3)
    assert sorted(set(cls.tolist())) == list(range(H.NCLS))
    v = H.bf16_to_f32(x).astype(np.float64) if kind == "bf16" else x.astype(np.float64)
    neg = np.signbit(v)
    K = H.KINDS[kind]
    unit = np.ldexp(1.0, H.EMIN[kind] - K["mant"])
    tiny = np.ldexp(1.0, H.EMIN[kind])
    vmax = (2.0 - np.ldexp(1.0, -K["mant"])) * np.ldexp(1.0, H.EMAX[kind])
    col = lambda name: v[:, cls == H.CLASSES.index(name)]  # noqa: E731
    sgn = lambda name: neg[:, cls == H.CLASSES.index(name)]  # noqa: E731
    assert (col("neg_zeros") == 0).all() and sgn("neg_zeros").all()
    assert (col("pos_then_neg_zero") == 0).all() and not sgn("pos_then_neg_zero")[0].any()
    assert sgn("pos_then_neg_zero")[1:].all()
    assert (np.isnan(col("one_nan")).sum(axis=0) == 1).all()
    a = col("inf_minus_inf")
    assert ((a == np.inf).sum(axis=0) == 1).all() and ((a == -np.inf).sum(axis=0) == 1).all()
    for name, v_inf in (("pos_inf", np.inf), ("neg_inf", -np.inf)):
        a = col(name)
        assert ((a == v_inf).sum(axis=0) == 1).all() and (np.isfinite(a).sum(axis=0) == n - 1).all()
    a = col("subnormals")
    assert (np.abs(a) <= 7 * unit).all() and (a != 0).any() and (a < 0).any() and (a > 0).any()
    a = col("into_subnormal")
    assert ((a == tiny).sum(axis=0) == 1).all() and ((a == -3 * unit).sum(axis=0) == 1).all()
    assert ((col("max_alone") == vmax).sum(axis=0) == 1).all()
    a = col("max_max_negmax")
    assert (a[0] == vmax).all() and (a[1] == vmax).all() and (a[2] == -vmax).all() and (a[3:] == 0).all()
    a = col("big_cancel")
    assert ((a == 2.0 ** 100).sum(axis=0) == 1).all() and ((a == -2.0 ** 100).sum(axis=0) == 1).all()
    assert ((a == 1.0).sum(axis=0) == n - 2).all()
    a = col("ties_to_even")
    assert (a[0] == 2.0 ** (K["mant"] + 1)).all() and (a[1:] == 1.0).all()
    a = col("ties_round_up")
    assert (a[0] == 2.0 ** (K["mant"] + 1) + 2).all() and (a[1:] == 1.0).all()
    a = col("max_plus_half_ulp")
    assert (a[0] == vmax).all() and (a[1] == 2.0 ** (H.EMAX[kind] - K["mant"] - 1)).all() and (a[2:] == 0).all()
    a = np.abs(col("wide_random"))
    assert a.min() < 2.0 ** -(K["exp_range"] - 8) and a.max() > 2.0 ** (K["exp_range"] - 8) and sgn("wide_random").any()
    a = col("uniform")
    assert (a >= -1).all() and (a < 1).all() and len(np.unique(a)) > min(a.size // 4, 400)
    a = col("exact_cancel")
    assert ((a == 1).sum(axis=0) == 1).all() and ((a == -1).sum(axis=0) == 1).all()
    # p and q fall on both sides of the 8-input group boundary
    where_nan = np.argmax(np.isnan(col("one_nan")), axis=0)
    assert (where_nan < 8).any() and (where_nan >= 8).any()


@pytest.mark.parametrize("kind", KINDS)
def test_deterministic_and_shift_moves_the_classes(kind):
    a = H.hostile(kind, 3, 500, shift=2, seed=4)
    H._hostile.cache_clear()
    b = H.hostile(kind, 3, 500, shift=2, seed=4)
    assert a is not b and a.tobytes() == b.tobytes()
    assert H.hostile(kind, 3, 500, shift=2, seed=5).tobytes() != a.tobytes()
    assert not a.flags.writeable  # shared among tests: nobody may change it
    # a sweep of the shift puts every class on every column
    seen = np.stack([H.class_of(40, s) for s in range(H.NCLS)])
    assert all(sorted(seen[:, i].tolist()) == list(range(H.NCLS)) for i in range(40))
    for near in (False, True):
        r = H.raw_bits(kind, 4, 300, seed=1, near=near)
        H._raw_bits.cache_clear()
        assert r.tobytes() == H.raw_bits(kind, 4, 300, seed=1, near=near).tobytes()
        assert r.dtype == _dtype(kind) and r.shape == (4, 300)
    for ik in ("u64", "i32"):
        assert H.wrapping(ik, 3, 100, 2).tobytes() == H.wrapping(ik, 3, 100, 2).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_raw_bits_near_keeps_exponents_close(kind):
    K = H.KINDS[kind]
    r = H.raw_bits(kind, 9, 4000, seed=3, near=True)
    e, _, top = H._fields(kind, r)
    d = np.abs(e.astype(np.int64)[1:] - e.astype(np.int64)[:1])
    assert d.max() <= 9 and len(np.unique(d)) == 10
    plain = H.raw_bits(kind, 9, 4000, seed=3)
    e2, _, _ = H._fields(kind, plain)
    assert e2.min() == 0 or K["bits"] == 64  # every exponent occurs (f64: 2048 of them, nearly)
    assert len(np.unique(e2)) > min(top, 250) * 0.9


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_numpy_on_hostile_inputs(oracle, kind, n):
    """The oracle on hostile inputs = the NumPy in-order restatement (f32,
    f64, bf16 native and bf16 wide), bit for bit, NaNs by NaN-ness."""
    dt = _dtype(kind)
    for i, x in enumerate(_arrays(kind, n)):
        got = oracle.reduce(list(x), dtype=dt)
        want = numpy_in_order(kind, x)
        assert bits_equal(got, want), (kind, n, i, first_mismatch(got, want))
        if kind == "bf16":
            gotw = oracle.reduce(list(x), dtype=dt, wide=True)
            wantw = numpy_in_order(kind, x, wide=True)
            assert bits_equal(gotw, wantw), (kind, n, i, "wide", first_mismatch(gotw, wantw))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_reference_on_hostile_inputs(oracle, kind, n):
    """... and = the reference's own reduce_kernel<T> (f32, f64, bf16 native)
    where oracle/_ref was built."""
    ref = _reference(kind)
    if ref is None:
        if os.path.exists(os.path.join(os.path.dirname(REF_SO), "BUILT_FROM_REFERENCE")):
            pytest.fail("tree built from the reference but oracle/_ref lacks the library for " + kind)
        pytest.skip("compiled reference only in the build container")
    for i, x in enumerate(_arrays(kind, n)):
        got = oracle.reduce(list(x), dtype=_dtype(kind))
        want = ref(x)
        assert bits_equal(got, want), (kind, n, i, first_mismatch(got, want))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_output_shares(oracle, kind, n):
    """NaN outputs are compared by NaN-ness only, so they stay under a
    quarter of every expected array; Inf, zero and subnormal outputs -- the
    ones a flush, a fold or a wrong rounding would change -- all occur."""
    dt = _dtype(kind)
    modes = [False, True] if kind == "bf16" else [False]
    for wide in modes:
        for shift in (0, 7):
            exp = oracle.reduce(list(H.hostile(kind, n, COUNT, shift=shift, seed=n)), dtype=dt, wide=wide)
            s = H.shares(kind, exp)
            H.assert_nan_cap(kind, exp)
            assert s["nan"] <= (1.5 if n == 1 else 2.5) / H.NCLS, s  # one_nan, and from two inputs inf_minus_inf
            assert s["inf"] > 2.0 / H.NCLS and s["zero"] > 1.5 / H.NCLS and s["sub"] > (0.5 if n == 1 else 1.5) / H.NCLS, s
        for near in (False, True):
            exp = oracle.reduce(list(H.raw_bits(kind, n, COUNT, seed=n, near=near)), dtype=dt, wide=wide)
            H.assert_nan_cap(kind, exp)


def test_bf16_subnormal_and_round_to_inf_expectations(oracle):
    """What the GPU must reproduce for bf16, stated as known answers: a
    subnormal input comes out unchanged, a sum of subnormals stays
    subnormal, the smallest normal minus 3 units is the subnormal 0x007D, and
    the largest bf16 plus half its ulp (2^119) is Inf in both accumulation
    modes."""
    x = np.array([[0x0001, 0x0003, 0x0080, 0x7F7F, 0x8005],
                  [0x0000, 0x0002, 0x8003, 0x7B00, 0x0002]], np.uint16)
    for wide in (False, True):
        assert oracle.reduce([x[0]], dtype=np.uint16, wide=wide).tolist() == x[0].tolist()
        assert oracle.reduce(list(x), dtype=np.uint16, wide=wide).tolist() == [0x0001, 0x0005, 0x007D, 0x7F80, 0x8003]


@pytest.mark.parametrize("kind", ["u64", "i32"])
def test_wrapping_integers_wrap(oracle, kind):
    """The integer inputs span the full range, most exact sums leave it, and
    the oracle returns them modulo 2^64 / 2^32 (Python integers as the
    independent statement)."""
    x = H.wrapping(kind, 9, 4099, seed=1)
    bits = 64 if kind == "u64" else 32
    exact = [sum(int(v) for v in col) for col in x.T]
    lo, hi = (0, 1 << 64) if kind == "u64" else (-(1 << 31), 1 << 31)
    assert int(x.min()) < lo + (hi - lo) // 100 and int(x.max()) > hi - (hi - lo) // 100
    assert np.mean([not lo <= s < hi for s in exact]) > 0.5
    got = [int(v) % (1 << bits) for v in oracle.reduce(list(x))]
    assert got == [s % (1 << bits) for s in exact]
