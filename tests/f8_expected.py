"""torch (CPU) restatement of the OCP FP8 reductions (a helper module, not a
conftest), shared by tests/test_f8_cpu.py and tests/test_f8_gpu.py.  It is
independent of the project's code: torch's own float8 conversions on the CPU
and explicit in-order folds over f32 tensors.

FP8 arrays are uint8 byte tensors.  ``fmt`` is "e4m3" (torch.float8_e4m3fn:
bias 7, max 448, no infinities, NaN (b & 0x7f) == 0x7f) or "e5m2"
(torch.float8_e5m2: bias 15, max 57344, infinities 0x7c / 0xfc, NaN above).

    widen(b)      the exact f32 value
    round_f(x)    NaN -> NaN; +-Inf -> +-Inf (e5m2) / NaN (e4m3); a finite x is
                  clamped to [-max, +max], then rounded to nearest even
    SUM native    acc = +0; acc = round_f(fl32(widen(acc) + widen(x))) per input
    SUM wide      an f32 accumulator from +0, round_f once at the end
    scaled        round_f(fl32(widen(s) * a32)) / wide round_f(fl32(s32 * a32))
    MAX / MIN     IEEE 754-2019 maximum / minimum of the widened values, from
                  the identity (e5m2 -Inf / +Inf, e4m3 0xfe / 0x7e)
"""
import torch

FORMATS = ("e4m3", "e5m2")
TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
CODE = {"e4m3": 16, "e5m2": 17}  # HICCL_FLOAT8_E4M3, HICCL_FLOAT8_E5M2
MAX = {"e4m3": 448.0, "e5m2": 57344.0}
MAX_ID = {"e4m3": 0xFE, "e5m2": 0xFC}  # the identity of a maximum
MIN_ID = {"e4m3": 0x7E, "e5m2": 0x7C}
ALPHAS = (0.5, -1.0, 0.0, 2.0 ** -20, 3e4, 1e38)  # the last two reach the clamp and, in f32, Inf

ALL_BYTES = torch.arange(256, dtype=torch.int32).to(torch.uint8)


def widen(b, fmt):
    return b.contiguous().view(TORCH[fmt]).float()


def round_f(x, fmt):
    assert x.dtype == torch.float32
    m = MAX[fmt]
    return torch.where(torch.isfinite(x), x.clamp(-m, m), x).to(TORCH[fmt]).view(torch.uint8)


def is_nan(b, fmt):
    low = b & 0x7F
    return low == 0x7F if fmt == "e4m3" else low > 0x7C


def a32(alpha):
    return torch.tensor(alpha, dtype=torch.float64).to(torch.float32)


def fold_sum(ins, fmt, wide=False, alpha=None, count=None):
    """ins: a list of uint8 tensors (n may be 0: pass count)."""
    count = ins[0].numel() if ins else count
    acc = torch.zeros(count, dtype=torch.float32)
    for x in ins:
        acc = acc + widen(x, fmt)
        if not wide:
            acc = widen(round_f(acc, fmt), fmt)
    if alpha is not None:
        acc = acc * a32(alpha)
    return round_f(acc, fmt)


def _mm(a, b, maximum):
    nan = torch.isnan(a) | torch.isnan(b)
    sa, sb = torch.signbit(a), torch.signbit(b)
    if maximum:
        take_b = (b > a) | ((b == a) & sa & ~sb)  # -0 < +0
    else:
        take_b = (b < a) | ((b == a) & ~sa & sb)
    return torch.where(nan, torch.full_like(a, float("nan")), torch.where(take_b, b, a))


def fold_mm(ins, fmt, maximum, count=None):
    count = ins[0].numel() if ins else count
    ident = (MAX_ID if maximum else MIN_ID)[fmt]
    acc = widen(torch.full((count,), ident, dtype=torch.uint8), fmt)
    for x in ins:
        acc = _mm(acc, widen(x, fmt), maximum)
    return round_f(acc, fmt)  # exact: the winner is an FP8 value


def expected(ins, fmt, op="sum", wide=False, alpha=None, count=None):
    if op == "sum":
        return fold_sum(ins, fmt, wide, alpha, count)
    return fold_mm(ins, fmt, op == "max", count)


def mismatches(got, exp, fmt):
    """Indices where got != exp, a NaN equal to any NaN."""
    gn, en = is_nan(got, fmt), is_nan(exp, fmt)
    return torch.nonzero((gn != en) | (~gn & (got != exp))).flatten()


def assert_equal(got, exp, fmt, what=""):
    got, exp = got.cpu().view(torch.uint8).flatten(), exp.flatten()
    assert got.numel() == exp.numel(), f"{what}: {got.numel()} elements, expected {exp.numel()}"
    bad = mismatches(got, exp, fmt)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {exp.numel()} differ, first at {i}: "
                             f"got {int(got[i]):#04x}, expected {int(exp[i]):#04x}")


def pair_table():
    """All 65,536 ordered pairs: a[i] = i >> 8, b[i] = i & 255."""
    i = torch.arange(65536, dtype=torch.int32)
    return (i >> 8).to(torch.uint8), (i & 255).to(torch.uint8)


def hostile_bytes(fmt, n, count, seed):
    """n inputs: random bytes salted with the hostile ones (NaNs, +-Inf or
    e4m3's NaN codes, +-max, subnormals, +-0), at seeded places."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    special = [0x00, 0x80, 0x01, 0x81, 0x07, 0x87, 0x7F, 0xFF, MIN_ID[fmt], MAX_ID[fmt], 0x7B, 0xFB, 0x7E, 0xFE,
               0x7C, 0xFC, 0x7D, 0x03, 0x83, 0x08, 0x04]
    sp = torch.tensor(special, dtype=torch.uint8)
    out = []
    for _ in range(n):
        x = torch.randint(0, 256, (count,), generator=g, dtype=torch.int32).to(torch.uint8)
        if count:
            mask = torch.rand(count, generator=g) < 0.25
            x = torch.where(mask, sp[torch.randint(0, len(special), (count,), generator=g)], x)
        out.append(x)
    return out


def tame_bytes(fmt, n, count, seed):
    """n inputs of small finite values (|x| <= 2): sums that do not all end in
    NaN or at the clamp."""
    g = torch.Generator().manual_seed(7000 * seed + n)
    return [round_f(torch.rand(count, generator=g) * 4 - 2, fmt) for _ in range(n)]
