#!/usr/bin/env python3
"""FP8 sums against bf16 on the flagship bytes, in alternating fresh processes.

    python tools/f8_ab.py --alternate 5 --out profiles/r11a_f8_ab.jsonl
    python tools/f8_ab.py --leg e4m3            (one leg, one JSON line)

The shape is config 2's bytes: n = 8 inputs of 1 GiB in the bucket layout
(hiccl_amd.bucket), under AUTO.  The legs are

    e4m3        hiccl_reduce on 8 x 2^30 torch.float8_e4m3fn, native accumulator
    e5m2        likewise on torch.float8_e5m2
    e4m3_wide   e4m3 with HICCL_ACC_WIDE (the f32 accumulator)
    bf16        8 x 2^29 bf16, native: the yardstick

Each leg runs in a process of its own (a child started by --alternate, under a
time limit; the parent process never opens the GPU): fill the inputs with
fill_uniform, `warmup` launches, then `steps` launches each between two device
events.  The line holds the median, minimum and maximum kernel time, the
bandwidth at the median ((n + 1) x bytes per buffer), AUTO's answer and a
sample check: 4,096 seeded elements of the output against the in-order fold of
the same elements of the inputs, restated with torch's conversions on the CPU.
DESIGN.md section 5, M21.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["e4m3", "e5m2", "e4m3_wide", "bf16"]


def run_leg(a):
    import torch
    sys.path.insert(0, ROOT)
    import hiccl_amd
    from hiccl_amd import _lib as L

    tdt = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2, "e4m3_wide": torch.float8_e4m3fn,
           "bf16": torch.bfloat16}[a.leg]
    esz = 2 if a.leg == "bf16" else 1
    count = (1 << a.log2bytes) // esz
    wide = a.leg.endswith("_wide")
    cfg = dict(acc=L.HICCL_ACC_WIDE) if wide else None
    dev = "cuda:0"
    ins, out = hiccl_amd.bucket(a.n, count, dtype=tdt, device=dev)
    for k, t in enumerate(ins):
        hiccl_amd.fill_uniform(t, 1234, k)
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        hiccl_amd.reduce(out, ins, config=cfg)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hiccl_amd.reduce(out, ins, config=cfg)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    idx = torch.randint(0, count, (4096,), generator=torch.Generator().manual_seed(7)).to(dev)
    got = out[idx].cpu()
    acc = torch.zeros(4096, dtype=torch.float32)
    for t in ins:
        acc = acc + t[idx].cpu().float()
        if not wide:
            acc = acc.to(tdt).float()  # in range: uniform [-1, 1) x 8 never reaches the FP8 clamp
    exp = acc.to(tdt)
    word = torch.uint8 if esz == 1 else torch.int16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    med = times[len(times) // 2]
    line = {"probe": "f8_ab", "leg": a.leg, "round": a.round, "n": a.n, "count": count, "layout": "bucket",
            "warmup": a.warmup, "steps": a.steps, "median_ms": round(med, 5), "min_ms": round(times[0], 5),
            "max_ms": round(times[-1], 5), "tbps_median": round((a.n + 1) * count * esz / med / 1e9, 4),
            "auto": hiccl_amd.auto_choice(tdt, count, a.n, config=cfg, cus=cus),
            "sample_ok": bool(torch.equal(got.view(word), exp.view(word))),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)


def alternate(a):
    lines = []
    legs = a.legs.split(",")
    for r in range(1, a.alternate + 1):
        for leg in legs:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg,
                   "--round", str(r), "--n", str(a.n), "--log2bytes", str(a.log2bytes), "--steps", str(a.steps),
                   "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a leg that failed or ran out of time ends the run: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"f8_ab: leg {leg} round {r} ended with status {p.returncode}")
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
    ap.add_argument("--legs", default=",".join(LEGS), help="the legs of a round, in order")
    ap.add_argument("--out", help="append the lines to this file")
    ap.add_argument("--round", type=int, default=1)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--log2bytes", type=int, default=30, help="bytes per input (default 1 GiB)")
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
