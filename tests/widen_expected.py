"""NumPy / torch (CPU) restatement of the widened sums (a helper module, not a
conftest), shared by tests/test_widen_cpu.py, tests/test_widen_gpu.py and
tests/golden/make_golden_widen.py.  Independent of the project's code:

    widen(x)   the exact f32 value of a bf16 / f16 / e4m3 / e5m2 element
               (bf16: the pattern shifted up; f16: NumPy's float16 -> float32;
               FP8: torch's own float8 -> float32 on the CPU, as a 256-entry table)
    s32        an explicit in-order loop of f32 adds from +0
    out        s32, or fl32(s32 * float32(alpha))

Inputs are uint16 (bf16, f16) or uint8 (FP8) bit patterns; outputs float32.
NaN outputs compare by NaN-ness.
"""
import hashlib

import numpy as np
import torch

import f8_expected as F8
import hostile as H32
import hostile_f16 as H16

KINDS = ("bf16", "f16", "e4m3", "e5m2")
HALVES = ("bf16", "f16")
CODE = {"bf16": 2, "f16": 6, "e4m3": 16, "e5m2": 17}  # HICCL_BFLOAT16, _FLOAT16, _FLOAT8_E4M3, _FLOAT8_E5M2
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
ESZ = {"bf16": 2, "f16": 2, "e4m3": 1, "e5m2": 1}
CARRIER = {"bf16": np.uint16, "f16": np.uint16, "e4m3": np.uint8, "e5m2": np.uint8}
COUNT = 17 * 241 + 5  # 4,102
NS = (1, 2, 3, 8, 9, 17)
NAN_CAP = H32.NAN_CAP

# name -> alpha (a double); the order is the fixtures' (key a<index>)
ALPHAS = (
    ("one", 1.0),
    ("half", 0.5),
    ("third", 1.0 / 3.0),
    ("-1/1024", -1.0 / 1024.0),
    ("2^-20", 2.0 ** -20),
    ("1e30", 1e30),
    ("zero", 0.0),
)

_F8_TABLE = {fmt: F8.widen(F8.ALL_BYTES, fmt).numpy().copy() for fmt in F8.FORMATS}


def a32(alpha):
    return np.float32(alpha)


def widen(kind, bits):
    """The exact f32 value of every element."""
    bits = np.asarray(bits, CARRIER[kind])
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    return _F8_TABLE[kind][bits]


def _f8_mix(fmt, n, count):
    """FP8 inputs whose widened sums stay mostly finite: f8_expected.tame_bytes
    with, per input, the hostile byte wherever a seeded uniform draw is below
    1 / (2n) -- about one hostile element in two columns, whatever n."""
    host = F8.hostile_bytes(fmt, n, count, seed=n)
    tame = F8.tame_bytes(fmt, n, count, seed=n)
    g = torch.Generator().manual_seed(9000 * n + F8.FORMATS.index(fmt))
    rows = []
    for k in range(n):
        take = torch.rand(count, generator=g) < 1.0 / (2 * n)
        rows.append(torch.where(take, host[k], tame[k]).numpy())
    return np.stack(rows) if rows else np.empty((0, count), np.uint8)


def inputs(kind, n, count=COUNT):
    """The (n, count) inputs of the fixtures and the GPU tests."""
    if n == 0:
        return np.empty((0, count), CARRIER[kind])
    if kind == "bf16":
        return H32.hostile("bf16", n, count)
    if kind == "f16":
        return H16.hostile(n, count)
    return _f8_mix(kind, n, count)


def acc_sum(kind, x, count=None):
    """s32: the in-order f32 sum of the widened (n, count) array `x` from +0."""
    x = np.asarray(x)
    count = x.shape[1] if x.ndim == 2 else count
    acc = np.zeros(count, np.float32)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            acc = acc + widen(kind, x[k])
    return acc


def finish(s, alpha):
    with np.errstate(all="ignore"):
        return (np.asarray(s, np.float32) * a32(alpha)).astype(np.float32)


def widened(kind, x, alpha=None, count=None):
    """The widened sum of `x`; alpha None: unscaled.  n == 0: +0, scaled a
    zero with alpha's sign."""
    s = acc_sum(kind, x, count)
    return s if alpha is None else finish(s, alpha)


def is_nan(a):
    return np.isnan(np.asarray(a, np.float32))


def assert_nan_cap(exp, inf_of=None):
    """Every expected array: at most a quarter NaN.

    `inf_of` (alpha = 0 only): the unscaled sum of the same inputs.  Inf * 0 is
    NaN, so under alpha = 0 the 2-byte kinds' hostile inputs (11.8 % NaN and
    17.6 % Inf sums for n >= 2) expect 29.4 % NaN, more than the cap.  A NaN
    that stands where `inf_of` is infinite is not counted: the caller compares
    that Inf bit for bit in the unscaled sum, so the position is pinned by an
    exact word and only its NaN-ness is left to this array."""
    nan = is_nan(exp)
    if inf_of is not None:
        nan = nan & ~np.isinf(np.asarray(inf_of, np.float32))
    s = float(nan.mean()) if np.size(exp) else 0.0
    assert s <= NAN_CAP, f"{s:.3f} of the expected f32 words are NaN (cap {NAN_CAP})"


def mismatches(got, exp):
    got, exp = np.asarray(got, np.float32).ravel(), np.asarray(exp, np.float32).ravel()
    gn, en = np.isnan(got), np.isnan(exp)
    return np.nonzero((gn != en) | (~gn & (got.view(np.uint32) != exp.view(np.uint32))))[0]


def bits_equal(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    return got.size == exp.size and len(mismatches(got, exp)) == 0


def assert_equal(got, exp, what=""):
    got, exp = np.asarray(got, np.float32).ravel(), np.asarray(exp, np.float32).ravel()
    assert got.size == exp.size, f"{what}: {got.size} words, expected {exp.size}"
    bad = mismatches(got, exp)
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {exp.size} words differ, first at {i}: got "
                             f"{got.view(np.uint32)[i]:#010x} ({got[i]!r}), expected {exp.view(np.uint32)[i]:#010x} "
                             f"({exp[i]!r})")


# ---- the every-pattern tables: input 0 every pattern of the type, input 1 one of 16 addends

ADDENDS = {
    # +-0, +-smallest subnormal, +-smallest normal, +-1, 1 + ulp, -256, +-max, 16, +-Inf, a NaN
    "bf16": np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080, 0x3F80, 0xBF80, 0x3F81, 0xC380, 0x7F7F, 0xFF7F,
                      0x4180, 0x7F80, 0xFF80, 0x7FC1], np.uint16),
    "f16": H16.ADDENDS,
    # +-0, +-smallest subnormal, +-smallest normal, +-1, 1 + ulp, -16, +-max, 2, the largest subnormal, the NaN codes
    "e4m3": np.array([0x00, 0x80, 0x01, 0x81, 0x08, 0x88, 0x38, 0xB8, 0x39, 0xD8, 0x7E, 0xFE, 0x40, 0x07, 0x7F, 0xFF],
                     np.uint8),
    # +-0, +-smallest subnormal, +-smallest normal, +-1, 1 + ulp, -16, +-max, 2, +-Inf, a NaN
    "e5m2": np.array([0x00, 0x80, 0x01, 0x81, 0x04, 0x84, 0x3C, 0xBC, 0x3D, 0xCC, 0x7B, 0xFB, 0x40, 0x7C, 0xFC, 0x7E],
                     np.uint8),
}
assert all(len(a) == 16 for a in ADDENDS.values())


def all_patterns(kind):
    bits = 8 * ESZ[kind]
    return np.arange(1 << bits, dtype=np.uint32).astype(CARRIER[kind])


def pattern_inputs(kind, i):
    """The two inputs of table row i: every pattern, and addend i everywhere."""
    p = all_patterns(kind)
    return np.stack([p, np.full_like(p, ADDENDS[kind][i])])


def patterns_expected(kind):
    """(16, 2^bits) f32 words: (+0 + widen(pattern)) + widen(addend i)."""
    return np.stack([widened(kind, pattern_inputs(kind, i)) for i in range(16)])


def words_hash(words):
    """sha256 of f32 words, every NaN replaced by one quiet NaN pattern."""
    w = np.ascontiguousarray(words, np.float32).view(np.uint32).copy()
    w[np.isnan(np.asarray(words, np.float32))] = 0x7FC00000
    return hashlib.sha256(w.astype("<u4").tobytes()).hexdigest()


def array_hash(a):
    """sha256 of an array's own bytes (the generated inputs)."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
