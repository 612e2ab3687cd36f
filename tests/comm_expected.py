"""What the eight collectives leave in every rank's receive buffer (a helper
module, not a conftest), shared by tests/test_types_comm_cpu.py and
tests/test_types_comm_gpu.py.

build/types_comm_{host,hip} (tests/cpp/types_comm.cpp) runs Comm<T> on raw
bytes; this module makes the send arrays and states, from the compositions of
hiccl_amd/csrc/compose.h and the known-answer test of include/hiccl/bench.h
alone (never from the schedule), what every element of every rank's receive
ALLOCATION must hold afterwards: the driver fills the allocation, GUARD
elements in front and behind included, with the byte 0xA5, and every element
the collective does not define must still hold it.

Arrays are unsigned bit patterns of the element's width (uint8 FP8, uint16
bf16 / f16, uint32 float / int32_t, uint64 double / size_t / uint64_t).

Inputs, so that no expectation depends on the order of a fold:
  gather, broadcast, all-to-all, all-gather   pure movement: hostile bit
      patterns (tests/hostile*.py, tests/f8_expected.py; FP8: every byte
      value), bit-identical on arrival;
  scatter, reduce, reduce-scatter, all-reduce  reductions (a scatter is a
      reduction of one sender, compose.h:25) --
      SUM     integers hashed from (rank, index), small enough that every
              partial sum of 8 ranks is exact in the type (SUM_LIMIT); int32_t
              and size_t take the full hash and wrap;
      MAX/MIN hostile values; a NaN compares by NaN-ness;
      PROD    +-2^-1 .. +-2^1 with a -0 on rank 0 per 17 elements;
      bitwise random words, mostly ones under AND, mostly zeros under OR.
No input element has every byte equal to 0xA5 (scrub); no integer-valued
float, no power of two and no MAX / MIN output (one of its inputs) then has,
and the tests assert it of every expected array (assert_no_prefill).

ordered_case(): all-reduce on the oracle's hashed uniform inputs, expected
from oracle/schedule.py's simulation of the reference schedule with the
type's own add -- the order of every sum, for every SUM type.
"""
import os
import sys

import numpy as np
import torch

import f8_expected as F8
import hostile as H
import hostile_f16 as H16
import ops_expected as OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import schedule as S  # noqa: E402

GUARD = 16      # tests/cpp/types_comm.cpp kGuard
PREFILL = 0xA5  # tests/cpp/types_comm.cpp kPrefill
ROOT_RANK = 0

GATHER, SCATTER, BROADCAST, REDUCE, ALLTOALL, ALLGATHER, REDUCESCATTER, ALLREDUCE = range(1, 9)
PATTERNS = tuple(range(1, 9))
MOVES = (GATHER, BROADCAST, ALLTOALL, ALLGATHER)

# driver type name -> (operator, kind)
TYPES = {
    "bf16": ("sum", "bf16"), "f16": ("sum", "f16"), "f8e4m3": ("sum", "e4m3"), "f8e5m2": ("sum", "e5m2"),
    "int32_t": ("sum", "i32"), "double": ("sum", "f64"), "float": ("sum", "f32"), "size_t": ("sum", "u64"),
    "maxof<bf16>": ("max", "bf16"), "minof<f16>": ("min", "f16"), "maxof<f8e4m3>": ("max", "e4m3"),
    "minof<f8e5m2>": ("min", "e5m2"), "maxof<int32_t>": ("max", "i32"), "minof<double>": ("min", "f64"),
    "prodof<bf16>": ("prod", "bf16"), "prodof<f16>": ("prod", "f16"), "bandof<int32_t>": ("band", "i32"),
    "borof<uint64_t>": ("bor", "u64"),
}
ORDERED_TYPES = ("bf16", "f16", "f8e4m3", "f8e5m2", "int32_t", "double")  # float: tests/test_mpi_*.py

BITS = {"e4m3": np.uint8, "e5m2": np.uint8, "bf16": np.uint16, "f16": np.uint16, "f32": np.uint32, "i32": np.uint32,
        "f64": np.uint64, "u64": np.uint64}
# |v| of the SUM inputs: 8 * limit is the largest integer below which every integer is a value of the type
SUM_LIMIT = {"e5m2": 1, "e4m3": 2, "bf16": 32, "f16": 256, "f32": 1 << 20, "f64": (1 << 40) - 1}
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f64": torch.float64,
         "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def is_nan(kind, bits):
    bits = np.asarray(bits)
    if kind in ("e4m3", "e5m2"):
        return F8.is_nan(torch.from_numpy(bits.astype(np.uint8)), kind).numpy()
    if kind == "f16":
        return H16.is_nan(bits)
    if kind in ("bf16", "f32", "f64"):
        return H.is_nan(kind, bits)
    return np.zeros(bits.shape, bool)


def prefilled(kind, shape):
    return np.frombuffer(bytes([PREFILL]) * (int(np.prod(shape)) * np.dtype(BITS[kind]).itemsize),
                         BITS[kind]).reshape(shape).copy()


def holds_prefill(kind, bits):
    """Elements whose every byte is 0xA5."""
    return np.asarray(bits) == prefilled(kind, (1,))[0]


def scrub(kind, bits):
    """The same array with the top byte of every all-0xA5 element turned into 0x25."""
    U = BITS[kind]
    top = U(0x80) << U(8 * (np.dtype(U).itemsize - 1))
    return np.where(holds_prefill(kind, bits), bits & ~top, bits).astype(U)


def assert_no_prefill(kind, defined):
    assert not holds_prefill(kind, defined).any(), "an expected element equals the 0xA5 prefill: pick another seed"


def _hash(np_, n, seed):
    """uint64 words hashed from (rank, element index, seed): splitmix64's finisher."""
    z = (np.arange(n, dtype=np.uint64)[None, :] * np.uint64(0x9E3779B97F4A7C15)
         + (np.arange(np_, dtype=np.uint64)[:, None] + np.uint64(1)) * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(seed))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _float_bits(kind, values):
    """float64 values (exactly representable) -> the kind's bits, through torch on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(values, np.float64))
    if kind in ("e4m3", "e5m2"):
        t = t.to(torch.float32)
    t = t.to(TORCH[kind])
    assert torch.equal(t.to(torch.float64), torch.from_numpy(np.ascontiguousarray(values, np.float64))), \
        f"a value is not exact in {kind}"
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy().view(
        BITS[kind]).copy()


# --------------------------------------------------------------- inputs ----

def move_inputs(kind, np_, n, seed):
    """(np_, n) hostile bit patterns: random bits in even columns (FP8: every
    byte value in turn), the hostile classes in odd ones."""
    col = np.arange(n)
    if kind in ("e4m3", "e5m2"):
        x = np.stack([t.numpy() for t in F8.hostile_bytes(kind, np_, n, seed)])
        raw = ((col[None, :] // 2 + 37 * np.arange(np_)[:, None]) & 0xFF).astype(np.uint8)
    elif kind == "bf16":
        x, raw = H.hostile("bf16", np_, n, seed, seed), H.raw_bits("bf16", np_, n, seed)
    elif kind == "f16":
        x, raw = H16.hostile(np_, n, seed, seed), H16.tamed_bits(np_, n, seed)
    elif kind in ("f32", "f64"):
        x, raw = H.hostile(kind, np_, n, seed, seed).view(BITS[kind]), H.raw_bits(kind, np_, n, seed).view(BITS[kind])
    else:
        x = raw = H.wrapping(kind, np_, n, seed).view(BITS[kind])
    return scrub(kind, np.where(col % 2 == 0, raw, x))


def reduce_inputs(op, kind, np_, n, seed):
    """(np_, n) bits for a reduction under `op`, and what fold() needs besides
    (SUM: the integer values)."""
    if op == "sum":
        h = _hash(np_, n, seed)
        if kind == "u64":
            return scrub(kind, h), None
        if kind == "i32":
            return scrub(kind, (h >> np.uint64(32)).astype(np.uint32)), None
        lim = SUM_LIMIT[kind]
        v = (h % np.uint64(2 * lim + 1)).astype(np.int64) - lim
        return _float_bits(kind, v.astype(np.float64)), v
    if op in ("max", "min"):
        if kind in ("e4m3", "e5m2"):
            # hostile_bytes alone leaves about half of an 8-rank fold NaN: keep the NaN codes in one
            # column of four (elsewhere their low bits are cleared: 0x7b / +-Inf)
            x = np.stack([t.numpy() for t in F8.hostile_bytes(kind, np_, n, seed)])
            tame = is_nan(kind, x) & (np.arange(n) % 4 != 0)[None, :]
            x = np.where(tame, x & np.uint8(0xFB if kind == "e4m3" else 0xFC), x)
        elif kind == "bf16":
            x = H.hostile("bf16", np_, n, seed, seed)
        elif kind == "f16":
            x = H16.hostile(np_, n, seed, seed)
        elif kind == "f64":
            x = H.hostile("f64", np_, n, seed, seed).view(np.uint64)
        else:
            x = OPS.int_cases(kind, np_, n, seed).view(BITS[kind])
        return scrub(kind, x), None
    if op == "prod":
        h = _hash(np_, n, seed)
        v = np.ldexp(1.0, (h % np.uint64(3)).astype(np.int64) - 1) * np.where((h >> np.uint64(8)) & np.uint64(1), -1.0, 1.0)
        v[0, np.arange(n) % 17 == 3] = -0.0
        return _float_bits(kind, v), None
    assert op in ("band", "bor") and kind in ("i32", "u64")
    a, b, c = (_hash(np_, n, seed + k) for k in (0, 101, 202))
    h = (a | b | c) if op == "band" else (a & b & c)
    return scrub(kind, h.astype(BITS[kind]) if kind == "u64" else (h >> np.uint64(32)).astype(np.uint32)), None


def fold(op, kind, bits, values=None):
    """The reduction of the rows of `bits` ((k, m), k >= 1) under `op`."""
    k = bits.shape[0]
    if op == "sum":
        if kind in ("u64", "i32"):
            return np.add.reduce(bits, axis=0, dtype=BITS[kind])  # wraps
        return _float_bits(kind, values.sum(axis=0).astype(np.float64))
    if op in ("max", "min"):
        if kind in ("e4m3", "e5m2"):
            return F8.fold_mm([torch.from_numpy(bits[r].copy()) for r in range(k)], kind, op == "max").numpy()
        carrier = OPS.carrier(kind)
        return np.ascontiguousarray(OPS.fold(kind, OPS.OPS[op], bits.view(carrier))).view(BITS[kind])
    if op == "prod":
        v = torch.from_numpy(bits.view({2: np.int16}[bits.itemsize]).copy()).view(TORCH[kind]).to(torch.float64).numpy()
        return _float_bits(kind, np.multiply.reduce(v, axis=0))
    return (np.bitwise_and if op == "band" else np.bitwise_or).reduce(bits, axis=0)


class Case:
    """One (type, pattern, ranks, count): every rank's send bits and the bits
    every rank's receive allocation must hold (`total` elements, the data at
    GUARD)."""

    def __init__(self, tname, pattern, np_, count, cmax, seed):
        op, kind = TYPES[tname]
        self.tname, self.kind, self.pattern, self.np_, self.count = tname, kind, pattern, np_, count
        n = count * np_
        values = None
        if pattern in MOVES:
            self.send = move_inputs(kind, np_, n, seed)
        else:
            self.send, values = reduce_inputs(op, kind, np_, n, seed)
        assert self.send.shape == (np_, n) and not holds_prefill(kind, self.send).any()
        send = self.send
        self.total = cmax * np_ + 2 * GUARD
        self.expected = prefilled(kind, (np_, self.total))
        self.defined = np.zeros((np_, self.total), bool)

        def put(rank, off, data):
            self.expected[rank, GUARD + off:GUARD + off + len(data)] = data
            self.defined[rank, GUARD + off:GUARD + off + len(data)] = True

        def red(ranks, lo, hi):
            rows = list(ranks)
            return fold(op, kind, send[rows, lo:hi], None if values is None else values[rows, lo:hi])

        everyone = range(np_)
        if pattern == GATHER:  # compose.h:22 -- rank p's first chunk to the root's chunk p
            for p in everyone:
                put(ROOT_RANK, p * count, send[p, :count])
        elif pattern == SCATTER:  # compose.h:25 -- the root's chunk p to rank p, a reduction of one sender
            for p in everyone:
                put(p, 0, red([ROOT_RANK], p * count, (p + 1) * count))
        elif pattern == BROADCAST:  # compose.h:28 -- the root's whole buffer to every rank, itself included
            for p in everyone:
                put(p, 0, send[ROOT_RANK])
        elif pattern == REDUCE:  # compose.h:31
            put(ROOT_RANK, 0, red(everyone, 0, n))
        elif pattern == ALLTOALL:  # compose.h:35 -- rank p's chunk q to rank q's chunk p
            for p in everyone:
                for q in everyone:
                    put(q, p * count, send[p, q * count:(q + 1) * count])
        elif pattern == ALLGATHER:  # compose.h:38
            for p in everyone:
                for q in everyone:
                    put(q, p * count, send[p, :count])
        elif pattern == REDUCESCATTER:  # compose.h:41
            for p in everyone:
                put(p, 0, red(everyone, p * count, (p + 1) * count))
        else:  # compose.h:44-46
            assert pattern == ALLREDUCE
            whole = red(everyone, 0, n)
            for p in everyone:
                put(p, 0, whole)


def ordered_case(tname, oracle, sch, np_, count, cmax):
    """All-reduce of the oracle's hashed uniform inputs (int32_t: the hash's
    words) on the initialised schedule `sch`: (send bits, expected allocation
    bits), the data region from oracle/schedule.py's simulation with the
    type's own add."""
    op, kind = TYPES[tname]
    assert op == "sum"
    n = count * np_
    add = None
    if kind == "f64":
        x = np.stack([oracle.fill(r + 1, n, 1234, np.float64)[r] for r in range(np_)])
        dtype = np.float64
    elif kind == "i32":
        x = (_hash(np_, n, 1234) >> np.uint64(32)).astype(np.uint32).view(np.int32)
        dtype = np.int32
    else:
        f = np.stack([oracle.fill(r + 1, n, 1234)[r] for r in range(np_)])
        if kind == "f16":
            x, dtype = f.astype(np.float16), np.float16
        elif kind == "bf16":
            x, dtype = np.stack([oracle.fill(r + 1, n, 1234, np.uint16)[r] for r in range(np_)]), np.uint16

            def add(acc, v):  # 0 + acc + v, rounded to bf16 after each add: acc is never -0
                return oracle.reduce([acc, v], dtype=np.uint16)
        else:
            x, dtype = np.stack([F8.round_f(torch.from_numpy(f[r]), kind).numpy() for r in range(np_)]), np.uint8

            def add(acc, v):
                return F8.fold_sum([torch.from_numpy(acc), torch.from_numpy(np.ascontiguousarray(v))], kind).numpy()
    user = {}
    for r in range(np_):
        user[(r, ("send",))] = np.ascontiguousarray(x[r])
        user[(r, ("recv",))] = prefilled(kind, (n,)).view(dtype)
    with np.errstate(over="ignore"):
        mem = S.simulate(sch, np_, user, dtype=dtype, add=add)
    total = cmax * np_ + 2 * GUARD
    expected = prefilled(kind, (np_, total))
    for r in range(np_):
        expected[r, GUARD:GUARD + n] = np.ascontiguousarray(mem[(r, ("recv",))]).view(BITS[kind])
    return np.ascontiguousarray(x).view(BITS[kind]), expected


def schedule_steps(np_, hier, libs, stripe, ring, depth, count):
    libmap = {"mpi": S.MPI, "ipc": S.IPC, "ipc_get": S.IPC_GET, "xccl": S.XCCL}
    sch = S.Schedule(np_, [int(h) for h in hier.split(",")], [libmap[lv] for lv in libs.split(",")],
                     numstripe=stripe, ringnodes=ring, pipedepth=depth, ring_reuse_fix=True)
    S.compose("allreduce", np_, count)(sch)
    return sch.init()


def mismatches(kind, got, exp):
    """Indices where got != exp; a NaN of a floating kind equals any NaN."""
    got, exp = np.asarray(got), np.asarray(exp)
    return np.nonzero((got != exp) & ~(is_nan(kind, got) & is_nan(kind, exp)))[0]


def describe(kind, got, exp, defined=None):
    bad = mismatches(kind, got, exp)
    if len(bad) == 0:
        return "no mismatch"
    i = int(bad[0])
    where = "" if defined is None else (" (defined by the collective)" if defined[i] else " (NOT defined by it: a stray write)")
    return (f"{len(bad)} of {len(exp)} elements differ, first at allocation index {i} = data index {i - GUARD}{where}: "
            f"got {int(got[i]):#x}, expected {int(exp[i]):#x}")


# ------------------------------------------------- one launch of the driver

ORDERED = "8o"  # the driver's token of the ordered all-reduce: pattern 8 under file names of its own


def _file(prefix, tname, count, token, rank):
    return f"{prefix}.{tname}.{count}.p{token}.rank{rank}.bin"


def tokens_of(tname, patterns=PATTERNS, ordered=True):
    """The driver's pattern list for `tname`: the patterns, and the ordered
    all-reduce for the types that have one."""
    return [str(p) for p in patterns] + ([ORDERED] if ordered and tname in ORDERED_TYPES else [])


def prepare(prefix, tname, np_, counts, tokens, oracle, topo):
    """Write every rank's send file for every (count, token) of one launch
    and return {(count, token): (expected, defined or None)}.  topo: (hier,
    libs, stripe, ring, depth), for the ordered all-reduce's schedule."""
    op, kind = TYPES[tname]
    cmax = max(counts)
    want = {}
    for count in counts:
        for token in tokens:
            if token == ORDERED:
                send, expected = ordered_case(tname, oracle, schedule_steps(np_, *topo, count), np_, count, cmax)
                defined = None
            else:
                case = Case(tname, int(token), np_, count, cmax, seed=int(token))
                send, expected, defined = case.send, case.expected, case.defined
                assert_no_prefill(kind, expected[defined])
                if op in ("max", "min") and kind not in ("i32", "u64") and count >= 64:
                    share = float(is_nan(kind, expected[defined]).mean())
                    assert share <= H.NAN_CAP, f"{share:.3f} of the expected {tname} outputs are NaN (cap {H.NAN_CAP})"
            for r in range(np_):
                send[r].tofile(_file(prefix, tname, count, token, r))
            want[(count, token)] = (expected, defined)
    return want


def judge(prefix, tname, np_, want):
    """Every rank's whole receive allocation of every (count, token) against
    `want`: movement bit for bit, reductions bit for bit with a NaN by
    NaN-ness, everything the collective does not define still 0xA5."""
    kind = TYPES[tname][1]
    failures = []
    for (count, token), (expected, defined) in want.items():
        exact = token != ORDERED and int(token) in MOVES
        for r in range(np_):
            got = np.fromfile(_file(prefix, tname, count, token, r), dtype=BITS[kind])
            if got.shape != expected[r].shape:
                failures.append(f"{tname} count {count} pattern {token} rank {r}: {got.size} elements, "
                                f"expected {expected[r].size}")
            elif exact and got.tobytes() != expected[r].tobytes():
                bad = np.nonzero(got != expected[r])[0]
                i = int(bad[0])
                failures.append(f"{tname} count {count} pattern {token} rank {r}: {len(bad)} elements differ, first at "
                                f"data index {i - GUARD}: got {int(got[i]):#x}, expected {int(expected[r][i]):#x}")
            elif len(mismatches(kind, got, expected[r])):
                failures.append(f"{tname} count {count} pattern {token} rank {r}: "
                                + describe(kind, got, expected[r], None if defined is None else defined[r]))
    assert not failures, f"{len(failures)} receive buffers wrong:\n" + "\n".join(failures[:12])
