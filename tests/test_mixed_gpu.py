"""GPU tier of the mixed plan kernels (hiccl_reduce_plan_add_unscaled: a scaled
plan whose computes are scaled one by one, k_reduce_plan_mixed), single process,
for the six floating dtypes and both accumulators where a dtype has two.

The yardsticks are the library's existing kernels on the same inputs: a scaled
compute of a mixed launch must write what a SCALED plan writes, an unscaled one
what a PLAIN plan writes, word for word, a NaN by NaN-ness; every byte around
an output stays the sentinel.

  1. one plan of five ragged computes (n, misalignment, count) = (2, 1, 1025),
     (9, V - 1, 2563), (17, 0, 255), (1, 1, 5), (0, 0, 33), V the elements of a
     packet, alternately scaled and unscaled, hostile inputs; TILE and PHASE,
     default (write-through by size) and nt stores, HICCL_PEER_LOADS; launched
     twice, then the scale changed, cleared and set again: the plan moves
     between the mixed, the plain and (a second plan, every compute unscaled /
     none unscaled) the scaled families with the right words each time;
  2. exhaustive: every 16-bit pattern (bf16, f16) and every byte (FP8) as the
     single input of an unscaled and of a scaled compute of one mixed plan,
     against the plain plan and the one-shot scaled call; f32 / f64 on the
     hostile sets;
  3. a mixed plan enqueued under torch.cuda.graph replays to the same words.
"""
import numpy as np
import pytest
import torch

import comm_expected as CE
import f8_expected as F8
import hiccl_amd
import hostile as H32
import hostile_f16 as H16
from hiccl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, PHASE = L.HICCL_ENGINE_TILE, L.HICCL_ENGINE_PHASE
WIDE, NATIVE = L.HICCL_ACC_WIDE, L.HICCL_ACC_NATIVE
NT = 2  # hiccl_reduce_config_t.store_policy: nt stores whatever the launch's size
SENTINEL = 0xA5
ALPHA = 0.7

# kind -> (torch dtype, bytes per element)
KINDS = {"f32": (torch.float32, 4), "f64": (torch.float64, 8), "bf16": (torch.bfloat16, 2), "f16": (torch.float16, 2),
         "e4m3": (torch.float8_e4m3fn, 1), "e5m2": (torch.float8_e5m2, 1)}
MODES = [pytest.param(k, w, id=f"{k}{'-wide' if w else ''}") for k in KINDS
         for w in ((False,) if k in ("f32", "f64") else (False, True))]
ENGINES = pytest.mark.parametrize("engine", [TILE, PHASE], ids=["tile", "phase"])
# name -> (peer flags, store_policy)
VARIANTS = {"default": (0, 0), "nt": (0, NT), "peer-loads": (L.HICCL_PEER_LOADS, 0),
            "peer-loads-stores": (L.HICCL_PEER_LOADS | L.HICCL_PEER_STORES, 0)}


def inputs(kind, n, count, seed):
    """(n, count) bit patterns: the existing hostile sets; FP8 sums of hostile
    bytes alone are nearly all NaN, so only input 0 is hostile there."""
    U = CE.BITS[kind]
    if n == 0:
        return np.empty((0, count), U)
    if kind in ("e4m3", "e5m2"):
        rows = [t.numpy() for t in F8.tame_bytes(kind, n, count, seed)]
        rows[0] = F8.hostile_bytes(kind, 1, count, seed)[0].numpy()
        return np.stack(rows)
    if kind == "f16":
        return np.ascontiguousarray(H16.hostile(n, count, shift=seed, seed=seed)).view(U)
    return np.ascontiguousarray(H32.hostile(kind, n, count, shift=seed, seed=seed)).view(U)


def aligned(t):
    """Bytes from t's start to its first 16-byte boundary."""
    return (16 - t.data_ptr() % 16) % 16


def place(kind, row, mis):
    """The row's bits `mis` elements past a 16-byte boundary of a buffer of its
    own: (uint8 tensor, element offset for Compute.add)."""
    esz = KINDS[kind][1]
    raw = torch.from_numpy(np.ascontiguousarray(row).view(np.uint8).copy())
    b = torch.full((raw.numel() + mis * esz + 48,), 0x5A, dtype=torch.uint8, device=DEV)
    off = aligned(b) + mis * esz
    b[off:off + raw.numel()] = raw.to(DEV)
    return b, off // esz


class Out:
    """An output of `count` elements `mis` elements past a 16-byte boundary, sentinels all around."""

    def __init__(self, kind, count, mis):
        self.kind, self.esz, self.count = kind, KINDS[kind][1], count
        self.buf = torch.empty(count * self.esz + mis * self.esz + 64, dtype=torch.uint8, device=DEV)
        self.off = aligned(self.buf) + mis * self.esz
        self.reset()

    def reset(self):
        self.buf.fill_(SENTINEL)

    def arg(self):
        return self.buf, self.off // self.esz

    def words(self, what):
        host = self.buf.cpu().numpy()
        end = self.off + self.count * self.esz
        assert (host[:self.off] == SENTINEL).all(), f"{what}: guard before the output written"
        assert (host[end:] == SENTINEL).all(), f"{what}: guard after the output written"
        return host[self.off:end].copy().view(CE.BITS[self.kind])


def same(kind, got, exp, what):
    assert got.shape == exp.shape, f"{what}: {got.shape} words, expected {exp.shape}"
    bad = CE.mismatches(kind, got, exp)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(exp)} words differ, first at {int(bad[0])}: "
                           f"got {int(got[bad[0]]):#x}, expected {int(exp[bad[0]]):#x}")


def plan(kind, wide, engine, variant="default", scale=None):
    peer, store = VARIANTS[variant]
    cfg = dict(engine=engine, acc=WIDE if wide else NATIVE)
    if store:
        cfg["store_policy"] = store
    comp = hiccl_amd.Compute(KINDS[kind][0], device=0, config=cfg, scale=scale)
    if peer:
        comp.set_peer(peer)
    return comp


def run(comp, outs):
    for o in outs:
        o.reset()
    comp.start()
    comp.wait()


# ------------------------------------------------- 1. five ragged computes

def ragged(kind):
    v = 16 // KINDS[kind][1]
    return [(2, 1, 1025), (9, v - 1, 2563), (17, 0, 255), (1, 1, 5), (0, 0, 33)]


UNSCALED = (False, True, False, True, False)  # alternately scaled and unscaled


@pytest.mark.parametrize("variant", list(VARIANTS))
@ENGINES
@pytest.mark.parametrize("kind,wide", MODES)
def test_five_ragged_computes_and_the_three_families(kind, wide, engine, variant):
    shapes = ragged(kind)
    xs = [inputs(kind, n, count, seed=c + 1) for c, (n, _, count) in enumerate(shapes)]
    ins = [[place(kind, r, (k + mis) % 3) for k, r in enumerate(x)] for x, (_, mis, _) in zip(xs, shapes)]
    plans, outs = {}, {}
    try:
        # the yardsticks (plain, scaled), the mixed plan, and a scaled plan whose computes are ALL unscaled
        for name, scale, flags in (("plain", None, None), ("scaled", ALPHA, None), ("mixed", ALPHA, UNSCALED),
                                   ("all-unscaled", ALPHA, (True,) * 5)):
            comp = plans[name] = plan(kind, wide, engine, variant, scale)
            outs[name] = [Out(kind, count, mis) for _, mis, count in shapes]
            for c, (n, _, count) in enumerate(shapes):
                if flags is None:
                    comp.add(ins[c], outs[name][c].arg(), count, compid=0)
                else:
                    comp.add(ins[c], outs[name][c].arg(), count, compid=0, unscaled=flags[c])
            assert comp.num_unscaled() == (sum(flags) if flags else 0)
            assert comp.numcomp == 5

        def yard(alpha):
            plans["scaled"].set_scale(alpha)
            run(plans["plain"], outs["plain"])
            run(plans["scaled"], outs["scaled"])
            return ([o.words("plain plan") for o in outs["plain"]], [o.words("scaled plan") for o in outs["scaled"]])

        def check(name, alpha, flags, step):
            plain, scaled = yard(alpha) if alpha is not None else (yard(ALPHA)[0], None)
            plans[name].set_scale(alpha)  # (None clears it)
            run(plans[name], outs[name])
            assert plans[name].engine() == engine
            telling = total = 0
            for c in range(5):  # the hostile sets stay under their NaN cap
                assert len(plain[c]) < 64 or CE.is_nan(kind, plain[c]).mean() <= H32.NAN_CAP, (c, CE.is_nan(kind, plain[c]).mean())
            for c in range(5):
                want = plain[c] if alpha is None or flags[c] else scaled[c]
                same(kind, outs[name][c].words(f"{name} compute {c}"), want,
                     f"{kind} {variant} {name} {step} alpha {alpha} compute {c} ({'un' if flags[c] else ''}scaled)")
                if alpha is not None and not flags[c]:
                    telling += int(((scaled[c] != plain[c]) & ~CE.is_nan(kind, plain[c])).sum())
                    total += len(plain[c])
            # the yardsticks themselves tell a scaled compute from a plain one
            assert alpha is None or alpha == 0.0 or telling * 8 >= total, (telling, total)

        for step in ("first launch", "second launch"):
            check("mixed", ALPHA, UNSCALED, step)
        check("all-unscaled", ALPHA, (True,) * 5, "plain family under a scale")
        # the scale flips on the launched plan: another alpha (the arguments alone), cleared (the plain
        # family), set again (the mixed family); the flags stay with the computes
        check("mixed", 1.0 / 3.0, UNSCALED, "alpha changed")
        check("mixed", None, UNSCALED, "scale cleared")
        check("mixed", ALPHA, UNSCALED, "scale set again")
        assert plans["mixed"].num_unscaled() == 2
        # and a plan launched plain first becomes a mixed one when it gets a scale
        check("all-unscaled", None, (True,) * 5, "cleared")
        sixth = Out(kind, shapes[0][2], 1)
        plans["all-unscaled"].add(ins[0], sixth.arg(), shapes[0][2], compid=0)  # compute 0's inputs, scaled
        plans["all-unscaled"].set_scale(ALPHA)
        plain, scaled = yard(ALPHA)
        run(plans["all-unscaled"], outs["all-unscaled"] + [sixth])
        same(kind, sixth.words("sixth"), scaled[0], f"{kind} {variant}: the sixth compute, scaled")
        for c in range(5):
            same(kind, outs["all-unscaled"][c].words("kept"), plain[c], f"{kind} {variant}: compute {c} stays plain")
    finally:
        for comp in plans.values():
            comp.close()


# ------------------------------------------------------------ 2. exhaustive

@ENGINES
@pytest.mark.parametrize("kind,wide", MODES)
def test_every_pattern_through_both_kinds_of_compute(kind, wide, engine):
    """n = 1: the unscaled compute of a mixed plan returns what the plain plan
    returns for every input word (the multiply by one is exact, or the contract
    would ask for a branch), the scaled one what hiccl_reduce_scaled returns."""
    U = CE.BITS[kind]
    if kind in ("bf16", "f16"):
        x = np.arange(1 << 16, dtype=np.uint32).astype(U)
    elif kind in ("e4m3", "e5m2"):
        x = np.tile(np.arange(256, dtype=np.uint32).astype(U), 3)
    else:
        x = inputs(kind, 1, 4102, seed=5)[0]
    count = len(x)
    src = [place(kind, x, 0)]
    cfg = dict(engine=engine, acc=WIDE if wide else NATIVE)
    for alpha in (ALPHA, 1.0 / 3.0, -2.0):
        mixed, plain = plan(kind, wide, engine, scale=alpha), plan(kind, wide, engine)
        try:
            o_un, o_sc, o_plain, o_one = (Out(kind, count, 0) for _ in range(4))
            mixed.add(src, o_un.arg(), count, compid=0, unscaled=True)
            mixed.add(src, o_sc.arg(), count, compid=0)
            plain.add(src, o_plain.arg(), count, compid=0)
            run(mixed, [o_un, o_sc])
            run(plain, [o_plain])
            t = o_one.buf[o_one.off:o_one.off + count * KINDS[kind][1]].view(KINDS[kind][0])
            s = src[0][0][src[0][1] * KINDS[kind][1]:][:count * KINDS[kind][1]].view(KINDS[kind][0])
            hiccl_amd.reduce(t, [s], count=count, config=cfg, scale=alpha)
            torch.cuda.synchronize()
            same(kind, o_un.words("unscaled"), o_plain.words("plain"), f"{kind} alpha {alpha}: unscaled compute vs plain plan")
            same(kind, o_sc.words("scaled"), o_one.words("one-shot"), f"{kind} alpha {alpha}: scaled compute vs one-shot")
        finally:
            mixed.close()
            plain.close()


# ---------------------------------------------------------------- 3. replay

@pytest.mark.parametrize("kind", ["f32", "bf16", "e4m3"])
def test_mixed_plan_replays_under_a_graph(kind):
    """The mixed launch is captured (after an eager launch uploaded the plan)
    and replayed on new input values; alpha and the flags travel with it."""
    shapes = ragged(kind)
    xs = [inputs(kind, n, count, seed=c + 11) for c, (n, _, count) in enumerate(shapes)]
    ins = [[place(kind, r, (k + mis) % 3) for k, r in enumerate(x)] for x, (_, mis, _) in zip(xs, shapes)]
    comps = {name: plan(kind, False, TILE, scale=scale) for name, scale in (("plain", None), ("scaled", ALPHA), ("mixed", ALPHA))}
    outs = {name: [Out(kind, count, mis) for _, mis, count in shapes] for name in comps}
    try:
        for name, comp in comps.items():
            for c, (n, _, count) in enumerate(shapes):
                comp.add(ins[c], outs[name][c].arg(), count, compid=0, unscaled=name == "mixed" and UNSCALED[c])
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            comps["mixed"].enqueue()  # warm-up outside capture: the upload
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            comps["mixed"].enqueue()
        for rep in range(2):
            for c, x in enumerate(xs):  # new values in the same buffers
                for (b, off), r in zip(ins[c], np.roll(x, rep + 1, axis=1)):
                    raw = torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).copy()).to(DEV)
                    b[off * KINDS[kind][1]:][:raw.numel()] = raw
            run(comps["plain"], outs["plain"])
            run(comps["scaled"], outs["scaled"])
            for o in outs["mixed"]:
                o.reset()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for c in range(5):
                want = outs["plain" if UNSCALED[c] else "scaled"][c].words("yardstick")
                same(kind, outs["mixed"][c].words(f"replay {rep}"), want, f"{kind} replay {rep} compute {c}")
    finally:
        torch.cuda.synchronize()
        for comp in comps.values():
            comp.close()
