"""NumPy restatement of the scaled sums (a helper module, not a conftest),
shared by tests/golden/make_golden_scale.py, tests/test_scale_cpu.py and
tests/test_scale_gpu.py.

    out[i] = finish(s[i], alpha)

``s`` is the plain SUM in the accumulator type -- the reference's in-order
``T acc = 0; acc += x`` (``wide=False``) or, for the 2-byte kinds, the in-order
f32 accumulator of HICCL_ACC_WIDE (``wide=True``).  ``alpha`` is a double and
``a32 = np.float32(alpha)`` (round to nearest even):

  * ``f64``: ``s * alpha``, one IEEE multiply;
  * ``f32``: ``s * a32``, one IEEE multiply;
  * ``bf16``, ``f16``: widen (exact), multiply in f32 ROUNDED TO F32, round to
    nearest even to the kind -- two roundings, which is the definition;
  * the same two wide: the f32 accumulator times a32, rounded to the kind.

bf16 and f16 arrays are uint16 bit patterns; the other kinds use their NumPy
dtype.  ``one_step`` is what the definition is NOT: the exact product rounded
once -- the every-pattern check keeps the two apart.
"""
import hashlib

import numpy as np

import hostile as H32
import hostile_f16 as H16
from ops_expected import ALL_PATTERNS, FLOATS, bits_equal, bits_of, carrier, first_mismatch, is_nan  # noqa: F401
from prod_expected import bf16_round, bf16_widen, canonical

KINDS = ("f32", "f64", "bf16", "f16")
HALVES = ("bf16", "f16")
COUNT = 17 * 241 + 5
NS = (1, 2, 3, 8, 9, 17)

# name -> alpha (a double); the order is the fixtures' (key a<index>)
ALPHAS = (
    ("one", 1.0),                  # cross-checks against the existing sum fixtures
    ("half", 0.5),
    ("0.7", 0.7),                  # separates two-step from one-step rounding (f16: 1,946 patterns)
    ("0.1", 0.1),                  # likewise (f16: 206)
    ("third", 1.0 / 3.0),
    ("-1/1024", -1.0 / 1024.0),
    ("three", 3.0),
    ("1+2^-24", 1.0 + 2.0 ** -24),  # a tie in double -> float: a32 == 1.0f, f64 multiplies by the double itself
    ("2^-20", 2.0 ** -20),
    ("1e30", 1e30),                # overflow in the narrowing
    ("zero", 0.0),
)
assert np.float32(ALPHAS[7][1]) == np.float32(1.0) and ALPHAS[7][1] != 1.0


def a32(alpha):
    return np.float32(alpha)


def hostile(kind, n, count=COUNT):
    """The fixtures' inputs: the existing hostile generators, shift = seed = n."""
    if n == 0:
        return np.empty((0, count), carrier(kind))
    return H16.hostile(n, count, shift=n, seed=n) if kind == "f16" else H32.hostile(kind, n, count, shift=n, seed=n)


def widen(kind, bits):
    """A 2-byte kind's patterns as f32 (exact)."""
    return bf16_widen(bits) if kind == "bf16" else np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def narrow(kind, f):
    """f32 -> the 2-byte kind's patterns, round to nearest even."""
    f = np.asarray(f, np.float32)
    with np.errstate(all="ignore"):
        return bf16_round(f) if kind == "bf16" else f.astype(np.float16).view(np.uint16)


def acc_sum(kind, x, wide=False, count=None):
    """The sum in the ACCUMULATOR type: f32 / f64 arrays; for the 2-byte kinds
    uint16 patterns (native) or the f32 accumulator (wide)."""
    x = np.asarray(x)
    n = x.shape[0]
    count = x.shape[1] if x.ndim == 2 else count
    with np.errstate(all="ignore"):
        if kind in ("f32", "f64"):
            acc = np.zeros(count, carrier(kind))
            for k in range(n):
                acc = acc + x[k]
            return acc
        if wide:
            acc = np.zeros(count, np.float32)
            for k in range(n):
                acc = acc + widen(kind, x[k])
            return acc
        acc = np.zeros(count, np.uint16)
        for k in range(n):
            acc = narrow(kind, widen(kind, acc) + widen(kind, x[k]))
        return acc


def plain_sum(kind, x, wide=False, count=None):
    """The unscaled SUM's output words."""
    s = acc_sum(kind, x, wide, count)
    return narrow(kind, s) if kind in HALVES and wide else s


def finish(kind, s, alpha, wide=False):
    """finish(s, alpha) of an accumulator array (acc_sum's)."""
    with np.errstate(all="ignore"):
        if kind == "f64":
            return np.asarray(s, np.float64) * np.float64(alpha)
        if kind == "f32":
            return np.asarray(s, np.float32) * a32(alpha)
        f = s if wide else widen(kind, s)
        p = (np.asarray(f, np.float32) * a32(alpha)).astype(np.float32)  # rounded to f32
        return narrow(kind, p)


def scaled(kind, x, alpha, wide=False, count=None):
    """The scaled sum of the (n, count) array `x`; n == 0 gives finish(+0, alpha)."""
    return finish(kind, acc_sum(kind, x, wide, count), alpha, wide)


def one_step(s, alpha):
    """NOT the definition: the exact product of the f16 patterns `s` and a32
    (35 significant bits at most: exact in a double) rounded ONCE to f16."""
    with np.errstate(all="ignore"):
        exact = widen("f16", s).astype(np.float64) * np.float64(a32(alpha))
        return exact.astype(np.float16).view(np.uint16)


def half_multiply(s, alpha):
    """NOT the definition either: a half multiply by (half)alpha."""
    with np.errstate(all="ignore"):
        return (np.asarray(s, np.uint16).view(np.float16) * np.float16(alpha)).astype(np.float16).view(np.uint16)


# ---- the every-pattern check: all 65,536 patterns as a single input, times every alpha

def patterns_expected(kind, wide=False):
    """(len(ALPHAS), 65536) words: input 0 every pattern, n = 1."""
    x = ALL_PATTERNS[None, :]
    return np.stack([scaled(kind, x, a, wide) for _, a in ALPHAS])


def words_hash(kind, words):
    """sha256 of uint16 words, NaNs canonicalised."""
    w = canonical(kind, words)
    return hashlib.sha256(np.ascontiguousarray(w).astype("<u2").tobytes()).hexdigest()


def array_hash(a):
    """sha256 of an array's own bytes (the generated inputs)."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
