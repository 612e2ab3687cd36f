"""Product-hostile inputs for the PROD parity tests.

The sum-hostile inputs of tests/hostile.py are wrong for products: seventeen
of them multiply to 0, Inf or NaN almost everywhere.  This module (a helper,
not a conftest) has the same interface -- ``hostile(kind, n, count, shift,
seed)`` returns an (n, count) array whose column i belongs to class
``(i + shift) % 17`` -- with classes made for a product, and the kinds
``f32``, ``f64`` (their NumPy dtypes), ``bf16`` and ``f16`` (uint16 bit
patterns).  Shared by tests/golden/make_golden_prod.py, tests/test_prod_cpu.py
and tests/test_prod_gpu.py.

M = explicit mantissa bits, emax / emin = largest / smallest normal exponent.
Only ``one_nan`` and ``inf_times_zero`` may produce a NaN: 2/17 of the outputs.
"""
import functools

import numpy as np

# explicit mantissa bits, emax, emin, the dtype the values are built in, the carrier of the result
KINDS = {
    "f32": dict(mant=23, emax=127, emin=-126, work=np.float32, dtype=np.float32, uint=np.uint32, bits=32, code=1),
    "f64": dict(mant=52, emax=1023, emin=-1022, work=np.float64, dtype=np.float64, uint=np.uint64, bits=64, code=2),
    "bf16": dict(mant=7, emax=127, emin=-126, work=np.float32, dtype=np.uint16, uint=np.uint16, bits=16, code=3),
    "f16": dict(mant=10, emax=15, emin=-14, work=np.float16, dtype=np.uint16, uint=np.uint16, bits=16, code=4),
}

CLASSES = (
    "near_one",          # random sign, full random mantissa, magnitude 2^u with u uniform in [-1, 1)
    "neg_zero_first",    # -0 as input 0, near_one elsewhere: the zero's sign is the sign product (1 x -0 = -0)
    "zero_at_p",         # +0 at a random position among signed near_one values
    "one_nan",           # a NaN at p
    "inf_times_zero",    # Inf at p, 0 at q: NaN (n = 1: Inf)
    "pos_inf",           # a lone +Inf among near_one values
    "neg_inf",           # a lone -Inf among near_one values
    "overflow_and_back", # 2^emax, 2, 2^-2 as inputs 0, 1, 2: Inf stays, the order decides
    "underflow_and_back",  # smallest normal, 2^-(M+2), 2^(M+2) as inputs 0, 1, 2: the middle step rounds to zero
    "into_subnormal",    # smallest normal with an odd mantissa times 0.75: a subnormal result that rounds
    "subnormal_scaled",  # a subnormal input times a power of two that makes it normal (flushed inputs show)
    "one_tie",           # 1 + k 2^-M (k odd) times 1.5, ones elsewhere: exactly half-way, rounds to even
    "max_alone",         # the largest finite value among ones
    "max_times_one_plus_ulp",  # max, then 1 + 2^-M: rounds to Inf
    "wide_pair",         # m 2^e at p and m' 2^-e at q, near_one elsewhere: far from 1 and back
    "small_integers",    # nonzero integers in -3 ... 3: exact while the product fits the significand
    "minus_ones",        # the sign is n's parity
)
NCLS = len(CLASSES)
assert NCLS == 17  # prime, as in tests/hostile.py
NAN_CLASSES = ("one_nan", "inf_times_zero")


def class_of(count, shift=0):
    """Class index of every column."""
    return (np.arange(count, dtype=np.int64) + shift) % NCLS


def _trunc_bf16(x):
    """f32 values cut to their top 16 bits (8 significant bits, exactly bf16)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def _near_one(kind, rng, shape):
    K = KINDS[kind]
    with np.errstate(all="ignore"):
        mag = np.exp2(rng.uniform(-1.0, 1.0, shape)).astype(K["work"])
    mag = np.minimum(mag, K["work"](2.0 - np.ldexp(1.0, -K["mant"])))  # a rounding up to 2.0 stays below it
    if kind == "bf16":
        mag = _trunc_bf16(mag)
    return mag * rng.choice([-1.0, 1.0], shape).astype(K["work"])


@functools.lru_cache(maxsize=128)
def _hostile(kind, n, count, shift, seed):
    K = KINDS[kind]
    W, M, emax, emin = K["work"], K["mant"], K["emax"], K["emin"]
    rng = np.random.default_rng([seed, n, count, shift, 40 + K["code"]])
    x = np.ones((n, count), W)
    cls = class_of(count, shift)
    p = rng.integers(0, n, count) if n else np.zeros(count, np.int64)
    q = (p + 1 + rng.integers(0, max(n - 1, 1), count)) % max(n, 1)  # != p whenever n >= 2
    two = lambda e: W(np.ldexp(1.0, e))  # noqa: E731  (exact powers of two, subnormal ones included)
    vmax = W((2.0 - np.ldexp(1.0, -M)) * np.ldexp(1.0, emax))
    if n == 0:
        return np.zeros((0, count), K["dtype"])

    def cols(name):
        return np.nonzero(cls == CLASSES.index(name))[0]

    def put(at, c, v):
        x[at[c], c] = v

    def mantissa(size, odd=False, below=1.0):
        """1 + k 2^-M with k uniform in [0, below 2^M), odd on request."""
        k = rng.integers(0, max(int(below * (1 << M)), 2), size)
        if odd:
            k |= 1
        return (1.0 + k.astype(np.float64) * np.ldexp(1.0, -M)).astype(W)

    for name in ("near_one", "neg_zero_first", "zero_at_p", "one_nan", "inf_times_zero", "pos_inf", "neg_inf",
                 "wide_pair"):
        c = cols(name)
        x[:, c] = _near_one(kind, rng, (n, len(c)))
    c = cols("neg_zero_first")
    x[0, c] = -0.0
    put(p, cols("zero_at_p"), 0.0)
    put(p, cols("one_nan"), np.nan)
    c = cols("inf_times_zero")
    put(p, c, np.inf)
    if n >= 2:
        put(q, c, 0.0)
    put(p, cols("pos_inf"), np.inf)
    put(p, cols("neg_inf"), -np.inf)
    c = cols("overflow_and_back")
    x[0, c] = two(emax)
    x[1:2, c] = 2.0
    x[2:3, c] = 0.25
    c = cols("underflow_and_back")
    x[0, c] = two(emin)
    x[1:2, c] = two(-(M + 2))
    x[2:3, c] = two(M + 2)
    c = cols("into_subnormal")
    put(p, c, W(1.0 + np.ldexp(1.0, -M)) * two(emin))
    if n >= 2:
        put(q, c, 0.75)
    c = cols("subnormal_scaled")
    put(p, c, rng.integers(1, 1 << M, len(c)).astype(W) * two(emin - M))
    if n >= 2:
        put(q, c, two(M + 3))
    c = cols("one_tie")  # 1.5 (1 + k 2^-M) < 2 needs k 2^-M < 1/3
    put(p, c, mantissa(len(c), odd=True, below=0.33))
    if n >= 2:
        put(q, c, 1.5)
    put(p, cols("max_alone"), vmax)
    c = cols("max_times_one_plus_ulp")
    x[0, c] = vmax
    x[1:2, c] = W(1.0 + np.ldexp(1.0, -M))
    c = cols("wide_pair")
    e = rng.integers(0, emax - 1, len(c))  # 0 ... emax - 2
    sign = rng.choice([-1.0, 1.0], (2, len(c))).astype(W)
    with np.errstate(all="ignore"):
        put(p, c, sign[0] * mantissa(len(c)) * np.exp2(e.astype(np.float64)).astype(W))
        if n >= 2:
            put(q, c, sign[1] * mantissa(len(c)) * np.exp2(-e.astype(np.float64)).astype(W))
    c = cols("small_integers")
    x[:, c] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (n, len(c))).astype(W)
    x[:, cols("minus_ones")] = -1.0
    if kind == "bf16":
        u = x.view(np.uint32)
        assert not (u & 0xFFFF).any(), "value not representable in bf16"
        out = (u >> 16).astype(np.uint16)
    elif kind == "f16":
        out = x.view(np.uint16)
    else:
        out = x
    out.setflags(write=False)
    return out


def hostile(kind, n, count, shift=0, seed=0):
    """(n, count) product-hostile inputs of `kind`; deterministic, cached, read-only."""
    return _hostile(kind, int(n), int(count), int(shift) % NCLS, int(seed))
