"""NumPy restatement of the PROD and bitwise reductions (a helper module, not
a conftest), shared by tests/golden/make_golden_prod.py, tests/test_prod_cpu.py
and tests/test_prod_gpu.py.

    out[i] = fold(op, identity, in[0][i], ..., in[n-1][i])     (list order)

PROD, identity 1, one multiply per input in the kind's own type:
  * ``f32``, ``f64``: the NumPy multiply of that dtype (IEEE, rounded to
    nearest even per step, subnormals kept);
  * ``f16``: NumPy's float16 multiply (widen, f32 multiply, round once: the
    half multiply's bits, since the f32 product of two halves is exact);
  * ``bf16``: widen both operands to f32 (exact), f32 multiply, round to
    nearest even ON THE BITS after every multiply;
  * ``i32``, ``u64``: wrap-around multiply, done on the unsigned view.
BAND / BOR / BXOR on ``i32`` and ``u64``: identities all-ones / 0 / 0.

bf16 and f16 arrays are uint16 bit patterns, as in tests/hostile_prod.py; the
other kinds use their NumPy dtype.  Comparison helpers (``bits_equal``, NaN by
NaN-ness) and the 16 two-input multipliers (``ADDENDS``) are ops_expected's.
"""
import hashlib

import numpy as np

from ops_expected import (ADDENDS, ALL_PATTERNS, FLOATS, INTS, bits_equal, bits_of, carrier,  # noqa: F401
                          first_mismatch, is_nan, nan_share)

PROD, BAND, BOR, BXOR = 16, 17, 18, 19
OPS = {"prod": PROD, "band": BAND, "bor": BOR, "bxor": BXOR}
BITWISE = {"band": BAND, "bor": BOR, "bxor": BXOR}
UINT = {"i32": np.uint32, "u64": np.uint64}


def ops_of(kind):
    """{name: code} of the new operators `kind` has."""
    return OPS if kind in INTS else {"prod": PROD}


def bf16_round(f):
    """f32 array -> bf16 bit patterns, round to nearest even; a NaN becomes the quiet NaN."""
    w = np.ascontiguousarray(f, np.float32).view(np.uint32)
    nan = (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (w.astype(np.uint64) + np.uint64(0x7FFF) + ((w >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)
    return np.where(nan, 0x7FC0, r & np.uint64(0xFFFF)).astype(np.uint16)


def bf16_widen(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def identity(kind, op):
    """The identity of `op` as a 0-d array of the kind's carrier dtype."""
    if kind in INTS:
        U = UINT[kind]
        v = {PROD: 1, BAND: np.iinfo(U).max, BOR: 0, BXOR: 0}[op]
        return np.array(v, U).view(INTS[kind])
    assert op == PROD, "the bitwise operators take the integer kinds only"
    if kind == "bf16":
        return np.array(0x3F80, np.uint16)
    if kind == "f16":
        return np.array(0x3C00, np.uint16)
    return np.array(1.0, carrier(kind))


def fold(kind, op, x, count=None):
    """The reduction of the (n, count) array `x`; n == 0 gives the identity
    (`count` elements)."""
    x = np.asarray(x)
    n = x.shape[0]
    count = x.shape[1] if x.ndim == 2 else count
    acc = np.full(count, identity(kind, op), carrier(kind))
    with np.errstate(all="ignore"):
        if kind in INTS:
            U = UINT[kind]
            a = acc.view(U)
            for k in range(n):
                b = np.ascontiguousarray(x[k]).astype(INTS[kind], copy=False).view(U)
                a = a * b if op == PROD else a & b if op == BAND else a | b if op == BOR else a ^ b
            return a.view(INTS[kind])
        assert op == PROD, "the bitwise operators take the integer kinds only"
        for k in range(n):
            if kind == "bf16":
                acc = bf16_round(bf16_widen(acc) * bf16_widen(x[k]))
            elif kind == "f16":
                acc = (acc.view(np.float16) * np.ascontiguousarray(x[k], np.uint16).view(np.float16)).view(np.uint16)
            else:
                acc = acc * x[k].astype(carrier(kind), copy=False)
    return acc


def int_cases(kind, n, count, seed=0):
    """(n, count) words of an integer kind, by column class (column mod 4):
    0 random words; 1 odd words only (a product of odd words keeps all its
    bits in play: it never collapses to zero); 2 random words with one of the
    extremes 0, 1, -1 (all-ones, UINT64_MAX), INT32_MIN (the top bit alone)
    at a random input; 3 single-bit and all-ones words."""
    T, U = INTS[kind], UINT[kind]
    bits = np.iinfo(U).bits
    rng = np.random.default_rng([seed, n, count, 29, 0 if kind == "i32" else 1])
    x = rng.integers(0, np.iinfo(U).max, (n, count), dtype=U, endpoint=True)
    if n == 0:
        return x.view(T)
    col = np.arange(count)
    x[:, col % 4 == 1] |= U(1)
    c = np.nonzero(col % 4 == 2)[0]
    special = np.array([0, 1, np.iinfo(U).max, 1 << (bits - 1)], U)
    x[rng.integers(0, n, len(c)), c] = special[rng.integers(0, len(special), len(c))]
    c = np.nonzero(col % 4 == 3)[0]
    one_bit = U(1) << rng.integers(0, bits, (n, len(c))).astype(U)
    x[:, c] = np.where(rng.integers(0, 4, (n, len(c))) == 0, np.iinfo(U).max, one_bit).astype(U)
    return x.view(T)


# ---- the every-pattern check: all 65,536 patterns times each of 16 multipliers

def canonical(kind, words):
    """uint16 words with every NaN replaced by the canonical quiet NaN."""
    M = FLOATS[kind][3]
    qnan = np.uint16((((1 << (15 - M)) - 1) << M) | (1 << (M - 1)))
    words = np.asarray(words, np.uint16)
    return np.where(is_nan(kind, words), qnan, words).astype(np.uint16)


def patterns_input(kind, a):
    """The (2, 65536) input of multiplier `a`: input 0 every pattern, input 1 the multiplier."""
    return np.stack([ALL_PATTERNS, np.full(1 << 16, ADDENDS[kind][a], np.uint16)])


def patterns_expected(kind):
    """(16, 65536) product words of every pattern times each multiplier."""
    return np.stack([fold(kind, PROD, patterns_input(kind, a)) for a in range(16)])


def patterns_hash(kind, words):
    """sha256 of the (16, 65536) words, NaNs canonicalised."""
    w = canonical(kind, words)
    assert w.shape == (16, 1 << 16)
    return hashlib.sha256(np.ascontiguousarray(w).astype("<u2").tobytes()).hexdigest()
