"""Hostile inputs and expected values for the fp16 (IEEE half) parity tests.

The half counterpart of tests/hostile.py (a helper module, not a conftest),
shared by tests/test_f16_cpu.py, tests/test_f16_gpu.py and
tests/golden/make_golden_f16.py.  Arrays are uint16 bit patterns.

``hostile(n, count, shift, seed)``: the 17 classes of hostile.CLASSES with the
same column scheme (class of column i = (i + shift) mod 17), built for half:
10 mantissa bits, exponents -14..15, smallest subnormal 2^-24, max 65504.
Only ``one_nan`` and ``inf_minus_inf`` yield NaN: 2/17 of the outputs.

``tamed_bits(n, count, seed, near)``: uniformly random 16-bit patterns; in
every column whose index is not a multiple of 8 the exponent field is reduced
modulo 29.  Untamed, 1/32 of half patterns are Inf / NaN and the sums
overflow, so 25-42 % of the outputs at n >= 9 are NaN and a comparison that
takes NaN by NaN-ness checks too little; tamed, at most about 5 % are, with
Inf and subnormal outputs still there (the untamed columns).

Expected values are NumPy restatements of the reduction:
``native_sum``  T acc = 0; acc += x[k] in half, in order (the reference's
                reduce_kernel<T> with T = _Float16 gives the same words:
                tests/golden/make_golden_f16.py checks it);
``wide_sum``    HICCL_ACC_WIDE: the same sum in float32, rounded once.
"""
import functools

import numpy as np

from hostile import CLASSES, NAN_CAP, NCLS, class_of  # noqa: F401  (re-exported)

MANT, EMIN, EMAX = 10, -14, 15
UNIT = np.float32(np.ldexp(1.0, EMIN - MANT))  # 2^-24, the smallest subnormal
VMAX = np.float32(65504.0)
WIDE_EXP = 12  # wide_random draws exponents over +-12

# The 16 addends of the exhaustive `+=` checks: +-0, +-2^-24, +-2^-14, +-1, 1 + 2^-10, -2048, +-65504, 16, +-Inf, a NaN
ADDENDS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x8400, 0x3C00, 0xBC00, 0x3C01, 0xE800, 0x7BFF, 0xFBFF,
                    0x4C00, 0x7C00, 0xFC00, 0x7E01], np.uint16)


def to_bits(x):
    """f32 values that are exactly half -> their uint16 bit patterns."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        h = x.astype(np.float16)
    back = h.astype(np.float32)
    assert ((back == x) | (np.isnan(back) & np.isnan(x))).all(), "value not representable in half"
    assert np.array_equal(np.signbit(back), np.signbit(x))
    return h.view(np.uint16)


def to_f32(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=128)
def _hostile(n, count, shift, seed):
    W = np.float32
    rng = np.random.default_rng([seed, n, count, shift, 4])
    x = np.zeros((n, count), W)
    cls = class_of(count, shift)
    p = rng.integers(0, n, count) if n else np.zeros(count, np.int64)
    q = (p + 1 + rng.integers(0, max(n - 1, 1), count)) % max(n, 1)  # != p whenever n >= 2
    two = lambda e: W(np.ldexp(1.0, e))  # noqa: E731
    if n == 0:
        return np.zeros((0, count), np.uint16)

    def cols(name):
        return np.nonzero(cls == CLASSES.index(name))[0]

    def put(at, c, v):
        x[at[c], c] = v

    c = cols("neg_zeros")
    x[:, c] = -0.0
    c = cols("pos_then_neg_zero")
    x[1:, c] = -0.0
    c = cols("one_nan")
    x[:, c] = rng.integers(-8, 9, (n, len(c))).astype(W)
    put(p, c, np.nan)
    c = cols("inf_minus_inf")
    x[:, c] = rng.integers(-8, 9, (n, len(c))).astype(W)
    put(p, c, np.inf)
    if n >= 2:
        put(q, c, -np.inf)
    for name, v in (("pos_inf", np.inf), ("neg_inf", -np.inf)):
        c = cols(name)
        x[:, c] = rng.integers(-8, 9, (n, len(c))).astype(W)
        put(p, c, v)
    c = cols("subnormals")  # |sum| <= 17 * 7 units < 2^7 units: an exact subnormal
    x[:, c] = rng.integers(-7, 8, (n, len(c))).astype(W) * UNIT
    c = cols("into_subnormal")
    put(p, c, two(EMIN))
    if n >= 2:
        put(q, c, W(-3.0) * UNIT)
    c = cols("max_alone")
    put(p, c, VMAX)
    c = cols("max_max_negmax")
    x[0, c] = VMAX
    x[1:2, c] = VMAX
    x[2:3, c] = -VMAX
    c = cols("big_cancel")  # 2^14 + 1 is not a half, so the order still decides
    x[:, c] = 1.0
    put(p, c, two(14))
    if n >= 2:
        put(q, c, -two(14))
    c = cols("ties_to_even")
    x[:, c] = 1.0
    x[0, c] = two(MANT + 1)
    c = cols("ties_round_up")
    x[:, c] = 1.0
    x[0, c] = two(MANT + 1) + W(2.0)
    c = cols("max_plus_half_ulp")  # 65504 + 16: a tie that rounds to Inf
    x[0, c] = VMAX
    x[1:2, c] = two(EMAX - MANT - 1)
    c = cols("wide_random")
    mant = 1.0 + rng.integers(0, 1 << MANT, (n, len(c))).astype(np.float64) * np.ldexp(1.0, -MANT)
    sign = rng.choice([-1.0, 1.0], (n, len(c)))
    x[:, c] = (sign * mant * np.exp2(rng.integers(-WIDE_EXP, WIDE_EXP + 1, (n, len(c))).astype(np.float64))).astype(W)
    c = cols("uniform")  # [-1, 1) on the 2^-23 grid, rounded to half (11 significant bits at every magnitude)
    u = (rng.integers(-(1 << 23), 1 << 23, (n, len(c))).astype(np.float64) * np.ldexp(1.0, -23)).astype(W)
    u = u.astype(np.float16).astype(W)
    x[:, c] = np.where(u >= 1.0, W(1.0) - two(-11), u)  # a draw that rounds up to 1.0 stays inside [-1, 1)
    c = cols("exact_cancel")
    x[:, c] = -0.0
    put(p, c, 1.0)
    if n >= 2:
        put(q, c, -1.0)
    out = to_bits(x).reshape(n, count)
    out.setflags(write=False)
    return out


def hostile(n, count, shift=0, seed=0):
    """(n, count) hostile half inputs (uint16 bits); deterministic, cached, read-only."""
    return _hostile(int(n), int(count), int(shift) % NCLS, int(seed))


@functools.lru_cache(maxsize=64)
def _tamed_bits(n, count, seed, near):
    rng = np.random.default_rng([seed, n, count, 7 + int(near), 4])
    u = rng.integers(0, 0xFFFF, (n, count), dtype=np.uint16, endpoint=True)
    emask = np.uint16(0x1F << MANT)
    if near and n > 1:  # as hostile.raw_bits: inputs 1.. take input 0's exponent +- 9
        e0 = ((u[0] & emask) >> MANT).astype(np.int64)
        e = np.clip(e0[None, :] + rng.integers(-9, 10, (n - 1, count)), 0, 31).astype(np.uint16)
        u[1:] = (u[1:] & ~emask) | (e << MANT)
    tame = np.arange(count) % 8 != 0
    e = ((u[:, tame] & emask) >> MANT) % 29
    u[:, tame] = (u[:, tame] & ~emask) | (e << MANT).astype(np.uint16)
    u.setflags(write=False)
    return u


def tamed_bits(n, count, seed=0, near=False):
    """Random half bit patterns, exponent field modulo 29 outside every
    eighth column (module docstring).  `near`: exponents within +-9 of input
    0's before the taming."""
    return _tamed_bits(int(n), int(count), int(seed), bool(near))


# ---- expected values

def native_sum(x, count=None):
    """T acc = 0; acc += x[k]: in-order half adds from +0, each rounded to half."""
    x = np.asarray(x, np.uint16)
    acc = np.zeros(x.shape[1] if x.ndim == 2 else count, np.float16)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            acc = (acc + x[k].view(np.float16)).astype(np.float16)
    return acc.view(np.uint16)


def wide_sum(x, count=None):
    """HICCL_ACC_WIDE: in-order float32 adds from +0, rounded to half once."""
    x = np.asarray(x, np.uint16)
    acc = np.zeros(x.shape[1] if x.ndim == 2 else count, np.float32)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            acc = acc + x[k].view(np.float16).astype(np.float32)
        return acc.astype(np.float16).view(np.uint16)


def expected(x, wide=False):
    return wide_sum(x) if wide else native_sum(x)


# ---- what an output holds

def is_nan(a):
    a = np.asarray(a, np.uint16)
    return ((a & 0x7C00) == 0x7C00) & ((a & 0x03FF) != 0)


def shares(a):
    """Fractions of NaN, Inf, zero and subnormal elements of `a`."""
    a = np.asarray(a, np.uint16)
    e, m = a & 0x7C00, a & 0x03FF
    size = max(a.size, 1)
    return dict(nan=float(((e == 0x7C00) & (m != 0)).sum()) / size, inf=float(((e == 0x7C00) & (m == 0)).sum()) / size,
                zero=float(((e == 0) & (m == 0)).sum()) / size, sub=float(((e == 0) & (m != 0)).sum()) / size)


def assert_nan_cap(exp):
    """Every expected array of the tests: at most a quarter NaN."""
    s = float(is_nan(exp).mean()) if np.size(exp) else 0.0
    assert s <= NAN_CAP, f"{s:.3f} of the expected f16 outputs are NaN (cap {NAN_CAP})"


def bits_equal(got, exp):
    """Bit for bit; a NaN output compares by NaN-ness only.  (conftest's
    bits_equal reads uint16 as bf16: its NaN mask does not fit half.)"""
    got, exp = np.asarray(got, np.uint16), np.asarray(exp, np.uint16)
    if got.shape != exp.shape:
        return False
    ng, ne = is_nan(got), is_nan(exp)
    return bool(np.array_equal(ng, ne) and np.array_equal(got[~ng], exp[~ne]))


def first_mismatch(got, exp):
    got, exp = np.asarray(got, np.uint16), np.asarray(exp, np.uint16)
    bad = np.nonzero((got != exp) & ~(is_nan(got) & is_nan(exp)))[0]
    if len(bad) == 0:
        return "no mismatch"
    i = bad[0]
    return f"{len(bad)} mismatches, first at {i}: got {int(got[i]):#06x} expected {int(exp[i]):#06x}"
