"""NumPy restatement of the accumulating widened sums (a helper module, not a
conftest), built on tests/widen_expected.py and shared by
tests/test_accum_cpu.py, tests/test_accum_gpu.py and
tests/golden/make_golden_accum.py.  Independent of the project's code:

    s32     widen_expected.acc_sum: the in-order f32 sum of the widened inputs
            from +0, FINISHED before the old output is looked at
    r       s32, or fl32(s32 * float32(alpha))
    out     fl32(p + r), p the old output; `times` launches fold the add:
            fl32(fl32(p + r) + r) ...

Three separately rounded f32 operations.  The variants a wrong kernel would
compute are here too, for the fixtures' conditions: `fused` (the product and
the add rounded once, an FMA), `prior_first` (p as addend 0 of the fold) and
`thrice_at_once` (p + 3r for three launches).
"""
import numpy as np

import widen_expected as W

KINDS = W.KINDS
NS = (0,) + W.NS  # 0, 1, 2, 3, 8, 9, 17
COUNT = W.COUNT

# name -> alpha (None: the unscaled form); the order is the fixtures' (key a<index>)
ALPHAS = (
    ("none", None),
    ("one", 1.0),
    ("third", 1.0 / 3.0),
    ("0.7", 0.7),
    ("-1/1024", -1.0 / 1024.0),
    ("zero", 0.0),
)

# the special words of a prior, at the columns col % 61 == 3 ... 11: the two
# zeros, the smallest positive and the largest negative subnormal, +-FLT_MAX,
# +-Inf, a NaN
SPECIALS = (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001)
NEG_ZERO = 0x80000000


def prior(kind, n, count=COUNT):
    """The old output of case (kind, n): uniform in [-2, 2) times 2^e, e uniform
    in -12 ... 12, seeded per (kind, n), with SPECIALS mixed in."""
    rng = np.random.default_rng([20261, KINDS.index(kind), n])
    v = (rng.random(count) * 4.0 - 2.0) * np.exp2(rng.integers(-12, 13, count).astype(np.float64))
    p = v.astype(np.float32)
    col = np.arange(count) % 61
    words = p.view(np.uint32)
    for i, w in enumerate(SPECIALS):
        words[col == 3 + i] = w
    return p


def contribution(kind, x, alpha=None, count=None):
    """r: the finished sum, scaled if alpha is given."""
    return W.widened(kind, x, alpha, count)


def add_prior(p, r, times=1):
    out = np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        for _ in range(times):
            out = (out + np.asarray(r, np.float32)).astype(np.float32)
    return out


def accumulated(kind, x, p, alpha=None, times=1):
    """The output after `times` launches on the old output p."""
    return add_prior(p, contribution(kind, x, alpha, len(p)), times)


def two_pass(p, s):
    """What the existing entries give for {p, s} -> p: the SAME-TYPE f32 sum
    (+0 + p) + s, which is p + s wherever p is not -0."""
    with np.errstate(all="ignore"):
        return ((np.float32(0.0) + np.asarray(p, np.float32)) + np.asarray(s, np.float32)).astype(np.float32)


def not_neg_zero(p):
    return np.asarray(p, np.float32).view(np.uint32) != NEG_ZERO


# ---- what a wrong kernel would compute

def fused(kind, x, p, alpha):
    """fma(s32, a32, p): the exact product plus p, rounded ONCE to f32.  The
    product of two f32 is exact in f64; the f64 sum is rounded to odd (TwoSum
    gives its error), so the final rounding to f32 is the single rounding of
    the exact value (53 >= 24 + 2 bits)."""
    s = W.acc_sum(kind, x, len(p)).astype(np.float64)
    with np.errstate(all="ignore"):
        prod = s * np.float64(W.a32(alpha))
        q = np.asarray(p, np.float32).astype(np.float64)
        t = prod + q
        bb = t - prod
        err = (prod - (t - bb)) + (q - bb)
        odd = (t.view(np.uint64) & np.uint64(1)).astype(bool)
        fix = np.isfinite(t) & np.isfinite(err) & (err != 0) & ~odd
        toward = np.where(err > 0, np.inf, -np.inf)
        t = np.where(fix, np.nextafter(t, toward), t)
        return t.astype(np.float32)


def prior_first(kind, x, p):
    """The unscaled fold with p as addend 0: ((p + x0) + x1) + ..."""
    acc = np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        for k in range(np.asarray(x).shape[0]):
            acc = (acc + W.widen(kind, x[k])).astype(np.float32)
    return acc


def thrice_at_once(kind, x, p, alpha):
    """p + 3r, the tripling rounded to f32."""
    r = contribution(kind, x, alpha, len(p))
    with np.errstate(all="ignore"):
        return (np.asarray(p, np.float32) + (np.float32(3.0) * r).astype(np.float32)).astype(np.float32)


# ---- the hand-written zero case: p = -0 and every input -0

ZERO_N, ZERO_COUNT = 3, 8


def zero_case(kind):
    """(inputs, prior): all -0.  Unscaled: s32 = +0 (the fold starts from +0),
    -0 + +0 = +0.  Under alpha = -1/1024: r = +0 * -2^-10 = -0, -0 + -0 = -0."""
    neg = 0x8000 if W.ESZ[kind] == 2 else 0x80
    x = np.full((ZERO_N, ZERO_COUNT), neg, W.CARRIER[kind])
    p = np.full(ZERO_COUNT, NEG_ZERO, np.uint32).view(np.float32)
    return x, p
