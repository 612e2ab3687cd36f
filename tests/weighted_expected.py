"""NumPy restatement of the weighted widened sums (a helper module, not a
conftest), built on tests/widen_expected.py and tests/accum_expected.py, which
stay as they are, and shared by tests/test_weighted_cpu.py,
tests/test_weighted_gpu.py and tests/golden/make_golden_weighted.py.
Independent of the project's code:

    t[k]    fl32(float32(w[k]) * widen(x[k])): ONE f32 multiply, rounded to f32
    s32     an explicit in-order loop of f32 adds of the rows t[k] from +0
    r       s32, or widen_expected.finish(s32, alpha)
    out     r, or accumulating accum_expected.add_prior(p, r)

The multiply and the add are two separately rounded operations.  The variant a
wrong kernel would compute is here too, for the fixtures' conditions: `fused`
(acc + w * x rounded once, an FMA).
"""
import numpy as np

import accum_expected as A
import widen_expected as W

KINDS = W.KINDS
NS = W.NS  # 1, 2, 3, 8, 9, 17
COUNT = W.COUNT
THIRD = 1.0 / 3.0

WEIGHT_SETS = ("ones", "dequant", "signs", "onezero", "extreme")
_EXTREME = (2.0 ** -20, 1e30, -1.0 / 1024.0, 3.0, 1.0 + 2.0 ** -23)

# (weight set, alpha) of the stored cases; the key of a case is <set>/<alpha name>
OVER_CASES = tuple((s, None) for s in WEIGHT_SETS) + (("dequant", THIRD), ("signs", THIRD))
ACCUM_CASES = tuple((s, a) for s in ("dequant", "signs", "extreme") for a in (None, THIRD))


def alpha_name(alpha):
    return "none" if alpha is None else "third"


def weights(name, n):
    """The n weights of a set: doubles rounded once to f32, k the input index."""
    k = np.arange(n, dtype=np.float64)
    if name == "ones":
        w = np.ones(n)
    elif name == "dequant":
        w = (0.7 + 0.1 * k) * np.exp2(-(np.arange(n) % 5).astype(np.float64))
    elif name == "signs":
        w = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 / 3.0 + k / 16.0)
    elif name == "onezero":
        w = 0.7 + 0.1 * k
        if n:
            w[n // 2] = 0.0
    elif name == "extreme":
        w = np.array([_EXTREME[i % 5] for i in range(n)], np.float64)
    else:
        raise KeyError(name)
    return w.astype(np.float32)


def rotated(w):
    """The weights permuted by one place: w[(k + 1) mod n]."""
    return np.roll(np.asarray(w, np.float32), -1)


def products(kind, x, w):
    """t: the (n, count) rows fl32(w[k] * widen(x[k]))."""
    x = np.asarray(x)
    w = np.asarray(w, np.float32)
    assert w.shape == (x.shape[0],), f"{w.shape} weights for {x.shape[0]} inputs"
    with np.errstate(all="ignore"):
        rows = [(W.widen(kind, x[k]) * np.float32(w[k])).astype(np.float32) for k in range(x.shape[0])]
    return np.stack(rows) if rows else np.empty((0,) + x.shape[1:], np.float32)


def acc_sum(kind, x, w, count=None):
    """s32: the in-order f32 sum of the products from +0."""
    x = np.asarray(x)
    count = x.shape[1] if x.ndim == 2 else count
    t = products(kind, x, w)
    acc = np.zeros(count, np.float32)
    with np.errstate(all="ignore"):
        for k in range(t.shape[0]):
            acc = (acc + t[k]).astype(np.float32)
    return acc


def weighted(kind, x, w, alpha=None, count=None):
    """The overwriting weighted sum; alpha None: unscaled."""
    s = acc_sum(kind, x, w, count)
    return s if alpha is None else W.finish(s, alpha)


def accumulated(kind, x, w, p, alpha=None, times=1):
    """The output after `times` accumulating launches on the old output p."""
    return A.add_prior(p, weighted(kind, x, w, alpha, len(p)), times)


def expected(kind, x, w, alpha=None, p=None):
    return weighted(kind, x, w, alpha) if p is None else accumulated(kind, x, w, p, alpha)


# ---- what a wrong kernel would compute

def fused(kind, x, w):
    """acc = fma(w[k], widen(x[k]), acc) in list order from +0: the exact
    product plus acc, rounded ONCE to f32.  The product of two f32 is exact in
    f64; the f64 sum is rounded to odd (TwoSum gives its error), so the final
    rounding to f32 is the single rounding of the exact value."""
    x = np.asarray(x)
    w = np.asarray(w, np.float32)
    acc = np.zeros(x.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            prod = W.widen(kind, x[k]).astype(np.float64) * np.float64(w[k])
            q = acc.astype(np.float64)
            t = prod + q
            bb = t - prod
            err = (prod - (t - bb)) + (q - bb)
            odd = (t.view(np.uint64) & np.uint64(1)).astype(bool)
            fix = np.isfinite(t) & np.isfinite(err) & (err != 0) & ~odd
            toward = np.where(err > 0, np.inf, -np.inf)
            t = np.where(fix, np.nextafter(t, toward), t)
            acc = t.astype(np.float32)
    return acc
