"""What an averaging Comm<T> (Comm<T>::set_scale) leaves in every rank's
receive allocation (a helper module, not a conftest), shared by
tests/test_avg_comm_cpu.py and tests/test_avg_comm_gpu.py.

build/avg_comm_{host,hip} (tests/cpp/avg_comm.cpp) is types_comm's driver with
set_scale(alpha) before the collective is composed.  The contract: every
element a scaled REDUCE defines holds finish(s, alpha), s the word the same
communicator leaves without the scale.  So this module takes
tests/comm_expected.py's expected allocations -- patterns 4 (reduce), 7
(reduce-scatter), 8 (all-reduce) from the compositions alone, and the ordered
all-reduce `8o` from oracle/schedule.py's simulation of the schedule -- and
applies `finish` to the elements the collective defines: scale_expected.finish
for f32 / f64 / bf16 / f16, f8_expected's scaled-sum restatement
(round_f(fl32(widen(s) * a32))) for the two FP8 kinds.  The all-gather half of
an all-reduce moves finished sums, so finish is applied once there too.
Everything else in the allocation must still be the 0xA5 prefill.

Token `r`: one add_reduce of `count` elements from the ranks of the other ring
node only to rank 0 (the receiver's node adds nothing); expected from
comm_expected.fold over the senders' rows.
Token with a suffix `c` (8c): clear_scale() before composing -- the unscaled words.
"""
import subprocess

import numpy as np
import torch

import comm_expected as CE
import f8_expected as F8
import scale_expected as SE

# driver type name -> kind; _Float16 is HICCL_FLOAT16 under the compiler's own type
TYPES = {"float": "f32", "double": "f64", "bf16": "bf16", "f16": "f16", "_Float16": "f16", "f8e4m3": "e4m3",
         "f8e5m2": "e5m2"}
CE_NAME = {"_Float16": "f16"}  # the comm_expected type with the same bits


def driver_types(mpirun, exe):
    """The types of TYPES the driver was built with: `_Float16` is there only
    where the compiler that built it has the type (the usage line lists them)."""
    p = subprocess.run([mpirun, "-np", "1", exe], capture_output=True, text=True, timeout=60, cwd="/tmp")
    listed = (p.stdout + p.stderr).split("types:")[-1].split()
    have = [t for t in TYPES if t in listed]
    assert set(TYPES) - set(have) <= {"_Float16"}, f"the driver lacks {set(TYPES) - set(have)}"
    return have


RING = "r"
ORDERED = CE.ORDERED
CLEARED = "8c"
SEED = {"4": 4, "7": 7, "8": 8, CLEARED: 8, RING: 29}
BIG = 4099  # the count at which the share of telling elements is checked


def finish(kind, bits, alpha):
    """finish(s, alpha) of the kind's bit patterns `bits` (any shape), native accumulator."""
    bits = np.ascontiguousarray(bits, CE.BITS[kind])
    if kind == "f32":
        return np.ascontiguousarray(SE.finish("f32", bits.view(np.float32), alpha)).view(np.uint32)
    if kind == "f64":
        return np.ascontiguousarray(SE.finish("f64", bits.view(np.float64), alpha)).view(np.uint64)
    if kind in ("bf16", "f16"):
        return np.asarray(SE.finish(kind, bits, alpha), np.uint16)
    t = torch.from_numpy(bits.reshape(-1).copy())
    return F8.round_f(F8.widen(t, kind) * F8.a32(alpha), kind).numpy().reshape(bits.shape)


def telling_share(kind, plain, alpha):
    """Share of the words `plain` whose finish differs both from the word itself
    (a missing multiply) and from finish(finish(s)) (a doubled one)."""
    once = finish(kind, plain, alpha)
    twice = finish(kind, once, alpha)
    nan = CE.is_nan(kind, once)
    return float(((once != plain) & (once != twice) & ~nan).mean())


def _ordered_f32(oracle, sch, np_, count, cmax):
    """comm_expected.ordered_case for float (which that module leaves to tests/test_mpi_*.py)."""
    n = count * np_
    x = np.stack([oracle.fill(r + 1, n, 1234)[r] for r in range(np_)]).astype(np.float32)
    user = {}
    for r in range(np_):
        user[(r, ("send",))] = np.ascontiguousarray(x[r])
        user[(r, ("recv",))] = CE.prefilled("f32", (n,)).view(np.float32)
    with np.errstate(over="ignore"):
        mem = CE.S.simulate(sch, np_, user, dtype=np.float32)
    expected = CE.prefilled("f32", (np_, cmax * np_ + 2 * CE.GUARD))
    for r in range(np_):
        expected[r, CE.GUARD:CE.GUARD + n] = np.ascontiguousarray(mem[(r, ("recv",))]).view(np.uint32)
    return np.ascontiguousarray(x).view(np.uint32), expected


def unscaled_case(tname, token, np_, count, cmax, oracle, topo, ring=1):
    """(send bits, expected allocation bits WITHOUT the scale, defined mask)."""
    kind = TYPES[tname]
    total = cmax * np_ + 2 * CE.GUARD
    if token == ORDERED:
        sch = CE.schedule_steps(np_, *topo, count)
        if kind == "f32":
            send, expected = _ordered_f32(oracle, sch, np_, count, cmax)
        else:
            send, expected = CE.ordered_case(CE_NAME.get(tname, tname), oracle, sch, np_, count, cmax)
        defined = np.zeros((np_, total), bool)
        defined[:, CE.GUARD:CE.GUARD + count * np_] = True
        return send, expected, defined
    if token == RING:
        n = count * np_
        send, values = CE.reduce_inputs("sum", kind, np_, n, SEED[RING])
        node = np_ // ring
        rows = list(range(node, min(2 * node, np_)))
        assert ring >= 2 and len(rows) >= 2, "token r needs two ring nodes of two ranks or more"
        expected = CE.prefilled(kind, (np_, total))
        defined = np.zeros((np_, total), bool)
        expected[0, CE.GUARD:CE.GUARD + count] = CE.fold("sum", kind, send[rows, :count], values[rows, :count])
        defined[0, CE.GUARD:CE.GUARD + count] = True
        return send, expected, defined
    case = CE.Case(CE_NAME.get(tname, tname), int(token.rstrip("c")), np_, count, cmax, seed=SEED[token])
    return case.send, case.expected, case.defined


def _file(prefix, tname, count, token, rank):
    return f"{prefix}.{tname}.{count}.p{token}.rank{rank}.bin"


def prepare(prefix, tname, np_, counts, tokens, oracle, topo, alpha):
    """Write every rank's send file for every (count, token) of one launch of
    build/avg_comm_* and return {(count, token): (expected, defined)}.
    topo: (hier, libs, stripe, ring, depth)."""
    kind = TYPES[tname]
    cmax = max(counts)
    want = {}
    for count in counts:
        for token in tokens:
            send, plain, defined = unscaled_case(tname, token, np_, count, cmax, oracle, topo, ring=topo[3])
            expected = plain.copy()
            if "c" not in token:
                expected[defined] = finish(kind, plain[defined], alpha)
                if count >= BIG:  # a condition on the inputs: the expectation alone tells the three outcomes apart
                    share = telling_share(kind, plain[defined], alpha)
                    assert share >= 0.5, (f"{tname} pattern {token} np {np_}: only {share:.3f} of the expected elements "
                                          "differ from both the unscaled word and the doubly scaled one")
            if token != ORDERED:  # the ordered inputs are the oracle's own, seed and all (as comm_expected.prepare)
                CE.assert_no_prefill(kind, expected[defined])
            assert (CE.holds_prefill(kind, expected[~defined])).all()
            for r in range(np_):
                send[r].tofile(_file(prefix, tname, count, token, r))
            want[(count, token)] = (expected, defined)
    return want


def judge(prefix, tname, np_, want):
    """Every rank's whole receive allocation against `want`, word for word, a
    NaN by NaN-ness; everything the collective does not define still 0xA5."""
    kind = TYPES[tname]
    failures = []
    for (count, token), (expected, defined) in want.items():
        for r in range(np_):
            got = np.fromfile(_file(prefix, tname, count, token, r), dtype=CE.BITS[kind])
            if got.shape != expected[r].shape:
                failures.append(f"{tname} count {count} pattern {token} rank {r}: {got.size} elements, "
                                f"expected {expected[r].size}")
            elif len(CE.mismatches(kind, got, expected[r])):
                failures.append(f"{tname} count {count} pattern {token} rank {r}: "
                                + CE.describe(kind, got, expected[r], defined[r]))
    assert not failures, f"{len(failures)} receive buffers wrong:\n" + "\n".join(failures[:12])
