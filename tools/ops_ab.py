#!/usr/bin/env python3
"""MAX, PROD or a scaled sum against SUM on the flagship shape, in alternating fresh processes.

    python tools/ops_ab.py --alternate 5 --out profiles/r09a_ops_ab.jsonl
    python tools/ops_ab.py --alternate 5 --legs sum,prod,prod_u64 --out profiles/r10a_ops_ab.jsonl
    python tools/ops_ab.py --alternate 5 --legs scaled,sum_same_shape,sum_then_mul --out profiles/r11a_scale_ab.jsonl
    python tools/ops_ab.py --leg max            (one leg, one JSON line)

The shape is config 2's: n = 8 inputs of 2^28 f32 in the bucket layout
(hiccl_amd.bucket), under AUTO.  The legs are

    sum   hiccl_reduce, the kernel every earlier measurement timed
    max   hiccl_reduce_op with HICCL_OP_MAX (untuned: AUTO's answer for it is
          recorded in the line)
    min   likewise with HICCL_OP_MIN
    prod  likewise with HICCL_OP_PROD
    prod_u64   HICCL_OP_PROD on 8 x 2^27 uint64 (the same bytes; random words,
          held in torch.int64 tensors: the same bits for either signedness)
    scaled   hiccl_reduce_scaled, f32, alpha = 1/8 (untuned: AUTO's answer for
          it, hiccl_reduce_auto_choice_scaled, is recorded in the line)
    sum_same_shape   SUM forced to the shape that answer names (engine, unroll,
          workgroups per CU, schedule, store form): the same launch without
          the finishing multiply
    sum_then_mul   SUM under AUTO, then a separate in-place multiply of the
          output by 1/8 (torch's mul_): the two passes a scaled sum replaces;
          both kernels lie between the two events

Each leg runs in a process of its own (a child started by --alternate, under a
time limit; the parent process never opens the GPU): fill the inputs with
fill_uniform, `warmup` launches, then `steps` launches each between two
device events.  The line holds the median, minimum and maximum kernel time,
the bandwidth at the median ((n + 1) x count x element bytes) and a sample
check: 4,096 seeded elements of the output against the in-order sum / product
/ the maximum of the same elements of the inputs (uniform [-1, 1): no NaN, no
zero of either sign, so NumPy's maximum states the expected word; the uint64
product wraps in NumPy as on the GPU; the scaled legs: the sum times 1/8 in
f32).  DESIGN.md section 5, M18, M19 and M20.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["sum", "max", "min", "prod", "prod_u64", "scaled", "sum_same_shape", "sum_then_mul"]
ALPHA = 0.125


def run_leg(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import hiccl_amd
    from hiccl_amd import _lib as L

    op = {"max": L.HICCL_OP_MAX, "min": L.HICCL_OP_MIN, "prod": L.HICCL_OP_PROD,
          "prod_u64": L.HICCL_OP_PROD}.get(a.leg, L.HICCL_OP_SUM)
    u64 = a.leg == "prod_u64"
    count = 1 << (a.log2count - 1 if u64 else a.log2count)  # the same bytes
    tdt, esz = (torch.int64, 8) if u64 else (torch.float32, 4)
    dev = "cuda:0"
    ins, out = hiccl_amd.bucket(a.n, count, dtype=tdt, device=dev)
    for k, t in enumerate(ins):
        if u64:
            t.random_(generator=torch.Generator(device=dev).manual_seed(1234 + k))  # 63 random bits per word
        else:
            hiccl_amd.fill_uniform(t, 1234, k)
    torch.cuda.synchronize()

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    scaled_auto = same_shape = None
    if a.leg in ("scaled", "sum_same_shape"):
        scaled_auto = hiccl_amd.auto_choice(tdt, count, a.n, cus=cus, scale=True)
    if a.leg == "sum_same_shape":
        same_shape = dict(engine=scaled_auto["engine"], unroll=scaled_auto["unroll"],
                          blocks_per_cu=scaled_auto["blocks_per_cu"], store_policy=scaled_auto["store_policy"],
                          schedule=L.HICCL_SCHED_DYNAMIC if scaled_auto["dynamic"] else L.HICCL_SCHED_STATIC)

    def launch():
        if a.leg == "scaled":
            hiccl_amd.reduce(out, ins, scale=ALPHA)
        elif a.leg == "sum_same_shape":
            hiccl_amd.reduce(out, ins, config=same_shape)
        elif a.leg == "sum_then_mul":
            hiccl_amd.reduce(out, ins)
            out.mul_(ALPHA)
        else:
            hiccl_amd.reduce(out, ins, op=op)  # SUM: hiccl_reduce itself

    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    idx = torch.from_numpy(np.random.default_rng(7).integers(0, count, 4096)).to(dev)
    got = out[idx].cpu().numpy()
    rows = np.stack([t[idx].cpu().numpy() for t in ins])
    if op == L.HICCL_OP_SUM:
        exp = np.zeros(len(got), np.float32)
        for r in rows:
            exp = (exp + r).astype(np.float32)
        if a.leg in ("scaled", "sum_then_mul"):
            exp = (exp * np.float32(ALPHA)).astype(np.float32)
    elif a.leg == "prod":
        exp = np.ones(len(got), np.float32)
        for r in rows:
            exp = (exp * r).astype(np.float32)
    elif u64:
        got, exp = got.view(np.uint64), np.ones(len(got), np.uint64)
        for r in rows:
            exp = exp * r.view(np.uint64)  # wraps
    else:
        exp = rows.max(axis=0) if a.leg == "max" else rows.min(axis=0)
    word = np.uint64 if u64 else np.uint32
    med = times[len(times) // 2]
    line = {"probe": "ops_ab", "leg": a.leg, "round": a.round, "n": a.n, "count": count, "layout": "bucket",
            "warmup": a.warmup, "steps": a.steps, "median_ms": round(med, 5), "min_ms": round(times[0], 5),
            "max_ms": round(times[-1], 5), "tbps_median": round((a.n + 1) * count * esz / med / 1e9, 4),
            "auto": scaled_auto if a.leg in ("scaled", "sum_same_shape") else
                    hiccl_amd.auto_choice(tdt, count, a.n, op=op, cus=cus),
            "sample_ok": bool(np.array_equal(got.view(word), exp.view(word))),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)


def alternate(a):
    lines = []
    legs = a.legs.split(",")
    for r in range(1, a.alternate + 1):
        for leg in legs:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg,
                   "--round", str(r), "--n", str(a.n), "--log2count", str(a.log2count), "--steps", str(a.steps),
                   "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a leg that failed or ran out of time ends the run: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"ops_ab: leg {leg} round {r} ended with status {p.returncode}")
            line = p.stdout.strip().splitlines()[-1]
            json.loads(line)
            lines.append(line)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
    med = lambda leg: sorted(json.loads(ln)["median_ms"] for ln in lines if json.loads(ln)["leg"] == leg)  # noqa: E731
    for leg in legs:
        v = med(leg)
        print(f"# {leg}: median of medians {v[len(v) // 2]:.4f} ms, range {v[0]:.4f}-{v[-1]:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--alternate", type=int, default=0, help="rounds of the legs, each leg in a fresh process")
    ap.add_argument("--legs", default="max,sum", help="the legs of a round, in order (default max,sum)")
    ap.add_argument("--out", help="append the lines to this file")
    ap.add_argument("--round", type=int, default=1)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--log2count", type=int, default=28)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    a = ap.parse_args()
    if any(leg not in LEGS for leg in a.legs.split(",")):
        ap.error(f"--legs: a comma list of {LEGS}")
    if a.alternate:
        alternate(a)
    elif a.leg:
        run_leg(a)
    else:
        ap.error("give --leg or --alternate")


if __name__ == "__main__":
    main()
