"""NumPy restatement of the MAX / MIN reductions (a helper module, not a
conftest), shared by tests/golden/make_golden_ops.py, tests/test_ops_cpu.py
and tests/test_ops_gpu.py.

    out[i] = fold(op, identity, in[0][i], ..., in[n-1][i])     (list order)

Floating kinds (``f32``, ``f64``, ``bf16``, ``f16``) follow IEEE 754-2019
maximum / minimum and are computed on the BIT PATTERNS, so that NaN and the
two zeros are handled here and not by whatever ``np.maximum`` does with them:

  * a pattern is NaN when its magnitude bits exceed Inf's; once an operand is
    NaN the result is NaN and stays NaN (the canonical quiet NaN is written);
  * every other pattern maps to a signed key ordered like its value: the
    magnitude bits for a clear sign, ``-magnitude - 1`` for a set one -- so
    -0 (key -1) is below +0 (key 0) and subnormals order like any value;
  * the fold starts from -Inf (MAX) or +Inf (MIN); nothing rounds.

Integer kinds: ``i32`` compares signed from INT32_MIN / INT32_MAX, ``u64``
unsigned from 0 / UINT64_MAX.

bf16 and f16 arrays are uint16 bit patterns, as in tests/hostile.py and
tests/hostile_f16.py; the other kinds use their NumPy dtype.
"""
import numpy as np

SUM, MAX, MIN = 0, 1, 2
OPS = {"max": MAX, "min": MIN}

# carrier dtype, unsigned view, total bits, explicit mantissa bits
FLOATS = {
    "f32": (np.float32, np.uint32, 32, 23),
    "f64": (np.float64, np.uint64, 64, 52),
    "bf16": (np.uint16, np.uint16, 16, 7),
    "f16": (np.uint16, np.uint16, 16, 10),
}
INTS = {"i32": np.int32, "u64": np.uint64}
KINDS = tuple(FLOATS) + tuple(INTS)


# The 16 addends of the exhaustive two-input checks.  f16: hostile_f16.ADDENDS
# (+-0, +-2^-24, +-2^-14, +-1, 1 + 2^-10, -2048, +-65504, 16, +-Inf, a NaN);
# bf16: the matching patterns (+-0, +-2^-133, +-2^-126, +-1, 1 + 2^-7, -2048,
# +-max, 16, +-Inf, a NaN).  The NaN is the last one.
F16_ADDENDS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x8400, 0x3C00, 0xBC00, 0x3C01, 0xE800, 0x7BFF, 0xFBFF,
                        0x4C00, 0x7C00, 0xFC00, 0x7E01], np.uint16)
BF16_ADDENDS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080, 0x3F80, 0xBF80, 0x3F81, 0xC500, 0x7F7F, 0xFF7F,
                         0x4180, 0x7F80, 0xFF80, 0x7FC1], np.uint16)
ADDENDS = {"f16": F16_ADDENDS, "bf16": BF16_ADDENDS}
ALL_PATTERNS = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def carrier(kind):
    return FLOATS[kind][0] if kind in FLOATS else INTS[kind]


def _layout(kind):
    _, U, B, M = FLOATS[kind]
    absmask = (1 << (B - 1)) - 1
    inf = ((1 << (B - 1 - M)) - 1) << M
    return U, B, M, absmask, inf


def bits_of(kind, a):
    """The unsigned bit patterns of a floating array of `kind`."""
    U = FLOATS[kind][1]
    return np.ascontiguousarray(a).view(U)


def is_nan(kind, a):
    U, B, M, absmask, inf = _layout(kind)
    return (bits_of(kind, a) & U(absmask)) > U(inf)


def _key(kind, bits):
    """Signed int64 key ordered like the (non-NaN) value: -0 < +0."""
    U, B, M, absmask, inf = _layout(kind)
    mag = (bits & U(absmask)).astype(np.int64)  # < 2^63 for every kind
    neg = (bits >> U(B - 1)).astype(bool)
    return np.where(neg, -mag - 1, mag)


def identity(kind, op):
    """The identity of `op` as a 0-d array of the kind's carrier dtype."""
    assert op in (MAX, MIN)
    if kind in INTS:
        info = np.iinfo(INTS[kind])
        return np.array(info.min if op == MAX else info.max, INTS[kind])
    U, B, M, absmask, inf = _layout(kind)
    bits = np.array(inf | ((1 << (B - 1)) if op == MAX else 0), U)
    return bits.view(carrier(kind))


def fold(kind, op, x, count=None):
    """The reduction of the (n, count) array `x`; n == 0 gives the identity
    (`count` elements)."""
    assert op in (MAX, MIN)
    x = np.asarray(x)
    n = x.shape[0]
    count = x.shape[1] if x.ndim == 2 else count
    if kind in INTS:
        x = x.astype(INTS[kind], copy=False)
        acc = np.full(count, identity(kind, op), INTS[kind])
        for k in range(n):  # integers: no NaN, no signed zero -- a plain compare
            take = x[k] > acc if op == MAX else x[k] < acc
            acc = np.where(take, x[k], acc)
        return acc
    U, B, M, absmask, inf = _layout(kind)
    qnan = U(inf | (1 << (M - 1)))
    acc = np.full(count, bits_of(kind, identity(kind, op)), U)
    nan = np.zeros(count, bool)
    for k in range(n):
        b = bits_of(kind, x[k])
        nan |= (b & U(absmask)) > U(inf)
        ka, kb = _key(kind, acc), _key(kind, b)
        take = kb > ka if op == MAX else kb < ka
        acc = np.where(take, b, acc)
    acc = np.where(nan, qnan, acc).astype(U)
    return acc.view(carrier(kind))


def bits_equal(kind, got, exp):
    """Bit for bit; a NaN output compares by NaN-ness only."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return False
    if kind in INTS:
        return bool(np.array_equal(got.astype(INTS[kind], copy=False), exp.astype(INTS[kind], copy=False)))
    g, e = bits_of(kind, got), bits_of(kind, exp)
    ng, ne = is_nan(kind, got), is_nan(kind, exp)
    return bool(np.array_equal(ng, ne) and np.array_equal(g[~ng], e[~ne]))


def first_mismatch(kind, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    if kind in INTS:
        bad = np.nonzero(got != exp)[0]
        g, e = got, exp
    else:
        g, e = bits_of(kind, got), bits_of(kind, exp)
        bad = np.nonzero((g != e) & ~(is_nan(kind, got) & is_nan(kind, exp)))[0]
    if len(bad) == 0:
        return "no mismatch"
    i = bad[0]
    return f"{len(bad)} mismatches, first at {i}: got {int(g[i]):#x} expected {int(e[i]):#x}"


def nan_share(kind, a):
    return float(is_nan(kind, a).mean()) if kind in FLOATS and np.size(a) else 0.0


def int_cases(kind, n, count, seed=0):
    """(n, count) random words of an integer kind mixed with the extremes,
    both identities and pairs that differ in the top bit only."""
    T = INTS[kind]
    info = np.iinfo(T)
    rng = np.random.default_rng([seed, n, count, 23, 0 if kind == "i32" else 1])
    x = rng.integers(info.min, info.max, (n, count), dtype=T, endpoint=True)
    if n == 0:
        return x
    top = 1 << (info.bits - 1)
    special = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1], T)
    col = np.arange(count)
    pick = col % 5 == 0
    x[rng.integers(0, n, count)[pick], col[pick]] = special[rng.integers(0, len(special), pick.sum())]
    if n >= 2:  # input 1 = input 0 with the top bit flipped
        flip = col % 7 == 3
        UT = np.uint32 if kind == "i32" else np.uint64
        x[1, flip] = (x[0, flip].view(UT) ^ UT(top)).view(T)
    return x


# ---- the every-pattern fixture (tests/golden/reduce_ops_patterns.npz)

def pattern_selector(kind, x, y):
    """Which input each output word of a two-input fold is: 0 input 0, 1 input
    1, 2 a NaN.  Asserts that every word is one of the three."""
    y = np.asarray(y, np.uint16)
    nan = is_nan(kind, y)
    sel = np.where(nan, 2, np.where(y == x[0], 0, 1)).astype(np.uint8)
    assert (nan | (y == x[0]) | (y == x[1])).all(), "an output that is neither input"
    return sel


def patterns_expected(kind, addend, sel):
    """The words a selector row stands for (a NaN as the canonical quiet NaN)."""
    U, B, M, absmask, inf = _layout(kind)
    qnan = np.uint16(inf | (1 << (M - 1)))
    return np.where(sel == 2, qnan, np.where(sel == 0, ALL_PATTERNS, np.uint16(addend))).astype(np.uint16)
