#!/usr/bin/env python3
"""One mixed plan launch against a scaled and a plain plan back to back, in
alternating fresh processes.

    python tools/mixed_ab.py --alternate 5 --out profiles/r14a_mixed_ab.jsonl
    python tools/mixed_ab.py --leg mixed            (one leg, one JSON line)

The step: 16 f32 computes of n = 2 inputs and 1 MiB each, every second one a
final compute of an averaging Comm<T> (scaled by alpha = 1/8), the others
intermediate (plain).  The legs are

    mixed   the 16 computes in ONE plan -- hiccl_reduce_plan_add for the final
            ones, hiccl_reduce_plan_add_unscaled for the others -- one launch of
            the mixed kernels;
    two     the yardstick, what the step costs without the per-compute flag:
            the 8 final computes in a scaled plan and the 8 others in a plain
            plan, enqueued back to back on one stream (only entries the ABI had
            before the flag: hiccl_reduce_plan_add, hiccl_reduce_plan_set_scale).

Each leg runs in a process of its own (a child started by --alternate, under a
time limit; the parent process never opens the GPU): fill the inputs with
fill_uniform, `warmup` steps, then `steps` steps each between two device events
on the stream.  The line holds the median, minimum and maximum time of a step
and a checksum of the outputs' words, which --alternate compares across legs.
The run-to-run spread of `two` over the rounds is the margin.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["two", "mixed"]


def run_leg(a):
    import torch
    sys.path.insert(0, ROOT)
    import hiccl_amd

    dev = "cuda:0"
    count = (a.kib << 10) // 4
    alpha = 1.0 / 8.0
    ins = [[torch.empty(count, dtype=torch.float32, device=dev) for _ in range(a.n)] for _ in range(a.computes)]
    outs = [torch.empty(count, dtype=torch.float32, device=dev) for _ in range(a.computes)]
    for c, row in enumerate(ins):
        for k, t in enumerate(row):
            hiccl_amd.fill_uniform(t, 1234, c * a.n + k)
    final = [c % 2 == 0 for c in range(a.computes)]
    plans = []
    if a.leg == "mixed":
        comp = hiccl_amd.Compute(torch.float32, device=0, scale=alpha)
        for c in range(a.computes):
            comp.add(ins[c], outs[c], count, compid=0, unscaled=not final[c])
        plans = [comp]
    else:
        scaled, plain = hiccl_amd.Compute(torch.float32, device=0, scale=alpha), hiccl_amd.Compute(torch.float32, device=0)
        for c in range(a.computes):
            (scaled if final[c] else plain).add(ins[c], outs[c], count, compid=0)
        plans = [scaled, plain]
    s = torch.cuda.current_stream()

    def step():
        for p in plans:
            p.enqueue(s)

    torch.cuda.synchronize()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    words = sum(int(o.view(torch.int32).to(torch.int64).sum().item()) for o in outs) & ((1 << 64) - 1)
    sample = all(torch.equal(outs[c], (ins[c][0] + ins[c][1]) * (alpha if final[c] else 1.0)) for c in range(a.computes)) \
        if a.n == 2 else None
    line = {"probe": "mixed_ab", "leg": a.leg, "round": a.round, "computes": a.computes, "n": a.n, "kib": a.kib,
            "final": sum(final), "launches_per_step": len(plans), "engines": [p.engine() for p in plans],
            "warmup": a.warmup, "steps": a.steps, "median_us": round(times[len(times) // 2], 3),
            "min_us": round(times[0], 3), "max_us": round(times[-1], 3), "checksum": words, "sample_ok": sample,
            "device": torch.cuda.get_device_name(0)}
    for p in plans:
        p.close()
    print(json.dumps(line), flush=True)


def alternate(a):
    lines = []
    legs = a.legs.split(",")
    for r in range(1, a.alternate + 1):
        for leg in legs:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg,
                   "--round", str(r), "--n", str(a.n), "--kib", str(a.kib), "--computes", str(a.computes),
                   "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a leg that failed or ran out of time ends the run: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"mixed_ab: leg {leg} round {r} ended with status {p.returncode}")
            line = p.stdout.strip().splitlines()[-1]
            json.loads(line)
            lines.append(line)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
    rows = [json.loads(ln) for ln in lines]
    if len({row["checksum"] for row in rows}) != 1:
        sys.exit("mixed_ab: the legs' outputs differ")
    for leg in legs:
        v = sorted(row["median_us"] for row in rows if row["leg"] == leg)
        print(f"# {leg}: median of medians {v[len(v) // 2]:.3f} us, range {v[0]:.3f}-{v[-1]:.3f} "
              f"(spread {v[-1] - v[0]:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--alternate", type=int, default=0, help="rounds of the legs, each leg in a fresh process")
    ap.add_argument("--legs", default=",".join(LEGS), help="the legs of a round, in order")
    ap.add_argument("--out", help="append the lines to this file")
    ap.add_argument("--round", type=int, default=1)
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--kib", type=int, default=1024, help="KiB per compute's output (default 1 MiB)")
    ap.add_argument("--computes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
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
