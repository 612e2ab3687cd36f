"""Hostile inputs for the parity tests: the values and shapes at which a
reduction kernel goes wrong without a uniform [-1, 1) test noticing.

A helper module (not a conftest), shared by tests/test_hostile_cpu.py (which
shows that the reference alone behaves as the GPU tests assume) and
tests/test_hostile_gpu.py (which runs the same arrays through every kernel).

``hostile(kind, n, count, shift, seed)`` returns an (n, count) array whose
column i belongs to class ``(i + shift) % NCLS``.  NCLS is prime, so along
the columns every class lands on every element slot of a 16-byte packet, on
every lane and on both halves of a packed bf16 pair; a sweep of ``shift``
over ``range(NCLS)`` puts every class on every single column (the scalar
head and tail of a short compute).  Where a class needs two distinct inputs
p != q they are drawn per column from a seeded generator, so with 9 and 17
inputs they fall on both sides of the kernels' 8-input group boundary.

Kinds: ``f32`` (float32), ``f64`` (float64), ``bf16`` (uint16 bit patterns;
every value is exactly representable in bf16).
"""
import functools

import numpy as np

# explicit mantissa bits, bits of the type, its NumPy carrier, the type the
# values are built in (bf16 values are built as f32 and truncated exactly)
KINDS = {
    "f32": dict(mant=23, bits=32, dtype=np.float32, work=np.float32, uint=np.uint32, code=1, exp_range=40),
    "f64": dict(mant=52, bits=64, dtype=np.float64, work=np.float64, uint=np.uint64, code=2, exp_range=60),
    "bf16": dict(mant=7, bits=16, dtype=np.uint16, work=np.float32, uint=np.uint16, code=3, exp_range=30),
}
EMAX, EMIN = {"f32": 127, "bf16": 127, "f64": 1023}, {"f32": -126, "bf16": -126, "f64": -1022}

CLASSES = (
    "neg_zeros",         # every input -0: the result is +0 (the accumulator starts at +0)
    "pos_then_neg_zero", # +0 first, then -0s
    "one_nan",           # one NaN at p, the rest finite
    "inf_minus_inf",     # +Inf at p, -Inf at q: NaN (n = 1: +Inf)
    "pos_inf",           # a lone +Inf among finite values
    "neg_inf",           # a lone -Inf
    "subnormals",        # small multiples of the smallest subnormal, both signs: a subnormal (or zero) sum
    "into_subnormal",    # smallest normal at p, -3 subnormal units at q: the sum drops below the normal range
    "max_alone",         # the largest finite value among zeros
    "max_max_negmax",    # max, max, -max in this order: Inf before the cancel
    "big_cancel",        # 2^100 at p, -2^100 at q, 1.0 elsewhere: the order decides
    "ties_to_even",      # 2^(mant + 1) first, then 1.0s: every add is a tie that rounds down
    "ties_round_up",     # 2^(mant + 1) + 2 first, then 1.0s: the ties alternate up and down
    "max_plus_half_ulp", # max, then half its ulp: a tie to even, i.e. Inf (bf16: the f32 sum is exact and the
                         # CONVERSION to bf16 ties to Inf)
    "wide_random",       # random sign, mantissa and exponent over +-exp_range
    "uniform",           # [-1, 1)
    "exact_cancel",      # 1.0 at p, -1.0 at q, -0 elsewhere: +0 (n = 1: 1.0)
)
NCLS = len(CLASSES)
assert NCLS == 17  # prime: see the module docstring


def class_of(count, shift=0):
    """Class index of every column."""
    return (np.arange(count, dtype=np.int64) + shift) % NCLS


def to_bf16_bits(x):
    """f32 values that are exactly bf16 -> their uint16 bit patterns."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "value not representable in bf16"
    return (u >> 16).astype(np.uint16)


def bf16_to_f32(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=64)
def _hostile(kind, n, count, shift, seed):
    K = KINDS[kind]
    W, M = K["work"], K["mant"]
    rng = np.random.default_rng([seed, n, count, shift, K["code"]])
    x = np.zeros((n, count), W)
    cls = class_of(count, shift)
    p = rng.integers(0, n, count) if n else np.zeros(count, np.int64)
    q = (p + 1 + rng.integers(0, max(n - 1, 1), count)) % max(n, 1)  # != p whenever n >= 2
    two = lambda e: W(np.ldexp(1.0, e))  # noqa: E731  (exact powers of two, subnormal ones included)
    unit = two(EMIN[kind] - M)           # smallest subnormal
    vmax = W((2.0 - np.ldexp(1.0, -M)) * np.ldexp(1.0, EMAX[kind]))
    if n == 0:
        return x

    def cols(name):
        return np.nonzero(cls == CLASSES.index(name))[0]

    def put(at, c, v):  # x[at[c], c] = v; with one input there is no second position
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
    c = cols("subnormals")  # |sum| <= 17 * 7 units < 128 units: subnormal (and exact) in bf16 too
    x[:, c] = rng.integers(-7, 8, (n, len(c))).astype(W) * unit
    c = cols("into_subnormal")
    put(p, c, two(EMIN[kind]))
    if n >= 2:
        put(q, c, W(-3.0) * unit)
    c = cols("max_alone")
    put(p, c, vmax)
    c = cols("max_max_negmax")
    x[0, c] = vmax
    x[1:2, c] = vmax
    x[2:3, c] = -vmax
    c = cols("big_cancel")
    x[:, c] = 1.0
    put(p, c, two(100))
    if n >= 2:
        put(q, c, -two(100))
    c = cols("ties_to_even")
    x[:, c] = 1.0
    x[0, c] = two(M + 1)
    c = cols("ties_round_up")
    x[:, c] = 1.0
    x[0, c] = two(M + 1) + W(2.0)
    c = cols("max_plus_half_ulp")
    x[0, c] = vmax
    x[1:2, c] = two(EMAX[kind] - M - 1)
    c = cols("wide_random")
    E = K["exp_range"]
    mant = 1.0 + rng.integers(0, 1 << M, (n, len(c))).astype(np.float64) * np.ldexp(1.0, -M)
    sign = rng.choice([-1.0, 1.0], (n, len(c)))
    x[:, c] = (sign * mant * np.exp2(rng.integers(-E, E + 1, (n, len(c))).astype(np.float64))).astype(W)
    c = cols("uniform")
    if kind == "f64":
        x[:, c] = rng.uniform(-1.0, 1.0, (n, len(c)))
    else:  # f32 on its 2^-23 grid; bf16: the same, truncated to bf16 (8 significant bits at every magnitude)
        u = (rng.integers(-(1 << 23), 1 << 23, (n, len(c))).astype(np.float64) * np.ldexp(1.0, -23)).astype(W)
        x[:, c] = (u.view(np.uint32) & np.uint32(0xFFFF0000)).view(W) if kind == "bf16" else u
    c = cols("exact_cancel")
    x[:, c] = -0.0
    put(p, c, 1.0)
    if n >= 2:
        put(q, c, -1.0)
    out = to_bf16_bits(x).reshape(n, count) if kind == "bf16" else x
    out.setflags(write=False)
    return out


def hostile(kind, n, count, shift=0, seed=0):
    """(n, count) hostile inputs of `kind`; deterministic, cached, read-only."""
    return _hostile(kind, int(n), int(count), int(shift) % NCLS, int(seed))


@functools.lru_cache(maxsize=32)
def _raw_bits(kind, n, count, seed, near):
    K = KINDS[kind]
    U, M, B = K["uint"], K["mant"], K["bits"]
    rng = np.random.default_rng([seed, n, count, 7 + int(near), K["code"]])
    hi = (1 << B) - 1
    u = rng.integers(0, hi, (n, count), dtype=U, endpoint=True)
    if near and n > 1:
        ebits = B - 1 - M
        emask = ((1 << ebits) - 1) << M
        e0 = ((u[0].astype(np.uint64) & np.uint64(emask)) >> np.uint64(M)).astype(np.int64)
        e = np.clip(e0[None, :] + rng.integers(-9, 10, (n - 1, count)), 0, (1 << ebits) - 1).astype(np.uint64)
        rest = u[1:].astype(np.uint64) & np.uint64(hi & ~emask)
        u[1:] = (rest | (e << np.uint64(M))).astype(U)
    out = u if kind == "bf16" else u.view(K["dtype"])
    out.setflags(write=False)
    return out


def raw_bits(kind, n, count, seed=0, near=False):
    """Every element a uniformly random bit pattern of the type.  `near`:
    inputs 1..n-1 take input 0's exponent +- 9, so the adds interact instead
    of the largest operand winning."""
    return _raw_bits(kind, int(n), int(count), int(seed), bool(near))


def wrapping(kind, n, count, seed=0):
    """Full-range integers whose sums wrap: `kind` u64 (uint64) or i32 (int32)."""
    rng = np.random.default_rng([seed, n, count, 11])
    if kind == "u64":
        return rng.integers(0, (1 << 64) - 1, (n, count), dtype=np.uint64, endpoint=True)
    assert kind == "i32"
    return rng.integers(-(1 << 31), (1 << 31) - 1, (n, count), dtype=np.int64, endpoint=True).astype(np.int32)


# ---- what an output holds (shares of NaN / Inf / zero / subnormal elements)

def _fields(kind, a):
    K = KINDS[kind]
    u = np.asarray(a).view(K["uint"]).astype(np.uint64)
    M, B = K["mant"], K["bits"]
    e = (u >> np.uint64(M)) & np.uint64((1 << (B - 1 - M)) - 1)
    m = u & np.uint64((1 << M) - 1)
    return e, m, (1 << (B - 1 - M)) - 1


def is_nan(kind, a):
    e, m, top = _fields(kind, a)
    return (e == top) & (m != 0)


def shares(kind, a):
    """Fractions of NaN, Inf, zero and subnormal elements of `a`."""
    e, m, top = _fields(kind, a)
    size = max(e.size, 1)
    return dict(nan=float(((e == top) & (m != 0)).sum()) / size, inf=float(((e == top) & (m == 0)).sum()) / size,
                zero=float(((e == 0) & (m == 0)).sum()) / size, sub=float(((e == 0) & (m != 0)).sum()) / size)


NAN_CAP = 0.25  # bits_equal compares a NaN output by NaN-ness only: keep those a minority


def assert_nan_cap(kind, expected):
    """Every expected array of the GPU tests: at most a quarter NaN."""
    s = float(is_nan(kind, expected).mean()) if np.size(expected) else 0.0
    assert s <= NAN_CAP, f"{s:.3f} of the expected {kind} outputs are NaN (cap {NAN_CAP})"
