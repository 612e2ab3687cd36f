#!/usr/bin/env python3
"""The weighted widened sum against the unweighted one and against what a caller
does today, in alternating fresh processes.

    python tools/weighted_ab.py --alternate 4 --out profiles/r15a_weighted_ab.jsonl
    python tools/weighted_ab.py --leg weighted --kind bf16     (one leg, one JSON line)

The shape is M22's: n = 8 inputs of 2^28 elements, bf16 or e4m3, summed into an
f32 output that is overwritten.  The legs are

    weighted  (a) one hiccl_reduce_weighted call: reduce_widened(out, ins, weights=w);
    widened   (b) the unweighted reduce_widened of the same buffers: the same
              bytes, so the gap to (a) is VALU time -- one multiply per element
              and input;
    twopass   (c) the caller's path without the weighted call: eight f32 copies
              x.float() * w[k], then the f32 reduce of the copies (only entries
              the package had before).

Each leg runs in a process of its own (a child started by --alternate, under a
time limit; the parent process never opens the GPU): fill the inputs with
fill_uniform, `warmup` steps, then `steps` steps each between two device events
on the stream.  The line holds the median, minimum and maximum time of a step
and a checksum of the output's words; --alternate checks that (a) and (c) wrote
the same words.  The spread of a leg over the rounds is the margin.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["weighted", "widened", "twopass"]
KINDS = ["bf16", "e4m3"]


def run_leg(a):
    import torch
    sys.path.insert(0, ROOT)
    import hiccl_amd

    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = "cuda:0"
    dtype = {"bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}[a.kind]
    count = 1 << a.log2_count
    ins = [torch.empty(count, dtype=dtype, device=dev) for _ in range(a.n)]
    for k, t in enumerate(ins):
        hiccl_amd.fill_uniform(t, 4321, k)
    out = torch.empty(count, dtype=torch.float32, device=dev)
    # dequantisation scales as an FP8 recipe has them: one per input, made on the device
    w = (0.7 + 0.1 * torch.arange(a.n, dtype=torch.float64)) * torch.exp2(-(torch.arange(a.n) % 5).double())
    w = w.float().to(dev)

    if a.leg == "weighted":
        def step():
            hiccl_amd.reduce_widened(out, ins, weights=w)
    elif a.leg == "widened":
        def step():
            hiccl_amd.reduce_widened(out, ins)
    else:
        def step():
            copies = [ins[k].float() * w[k] for k in range(a.n)]
            hiccl_amd.reduce(out, copies)

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
        times.append(e0.elapsed_time(e1))
    times.sort()
    words = int(out.view(torch.int32).to(torch.int64).sum().item()) & ((1 << 64) - 1)
    in_bytes = a.n * count * ins[0].element_size()
    line = {"probe": "weighted_ab", "leg": a.leg, "kind": a.kind, "round": a.round, "n": a.n, "log2_count": a.log2_count,
            "warmup": a.warmup, "steps": a.steps, "median_ms": round(times[len(times) // 2], 4),
            "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4),
            "one_pass_bytes": in_bytes + 4 * count, "checksum": words, "nan": int(torch.isnan(out).sum().item()),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)


def alternate(a):
    rows = []
    for r in range(1, a.alternate + 1):
        for kind in a.kinds.split(","):
            for leg in a.legs.split(","):
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg,
                       "--kind", kind, "--round", str(r), "--n", str(a.n), "--log2-count", str(a.log2_count),
                       "--steps", str(a.steps), "--warmup", str(a.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:  # a leg that failed or ran out of time ends the run: nothing more is started
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit(f"weighted_ab: leg {leg} {kind} round {r} ended with status {p.returncode}")
                line = p.stdout.strip().splitlines()[-1]
                rows.append(json.loads(line))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as fh:
                        fh.write(line + "\n")
    for kind in a.kinds.split(","):
        mine = [row for row in rows if row["kind"] == kind]
        sums = {row["checksum"] for row in mine if row["leg"] in ("weighted", "twopass")}
        if len(sums) > 1:
            sys.exit(f"weighted_ab: {kind}: the weighted call and the two-pass path wrote different words")
        med = {}
        for leg in a.legs.split(","):
            v = sorted(row["median_ms"] for row in mine if row["leg"] == leg)
            if v:
                med[leg] = v
                print(f"# {kind} {leg}: median of medians {v[len(v) // 2]:.4f} ms, range {v[0]:.4f}-{v[-1]:.4f} "
                      f"(spread {v[-1] - v[0]:.4f})", flush=True)
        if "weighted" in med and "twopass" in med:
            pairs = [(x["median_ms"], y["median_ms"]) for x in mine if x["leg"] == "weighted"
                     for y in mine if y["leg"] == "twopass" and y["round"] == x["round"]]
            print(f"# {kind}: weighted faster than two-pass in {sum(x < y for x, y in pairs)} of {len(pairs)} pairs",
                  flush=True)
        if "weighted" in med and "widened" in med:
            ratios = sorted(x["median_ms"] / y["median_ms"] for x in mine if x["leg"] == "weighted"
                            for y in mine if y["leg"] == "widened" and y["round"] == x["round"])
            print(f"# {kind}: weighted / widened per pair {', '.join(f'{q:.4f}' for q in ratios)}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--kind", choices=KINDS, default="bf16")
    ap.add_argument("--alternate", type=int, default=0, help="rounds of the legs, each leg in a fresh process")
    ap.add_argument("--legs", default=",".join(LEGS), help="the legs of a round, in order")
    ap.add_argument("--kinds", default=",".join(KINDS), help="the input types of a round, in order")
    ap.add_argument("--out", help="append the lines to this file")
    ap.add_argument("--round", type=int, default=1)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--log2-count", type=int, default=28, help="log2 of the elements per input (default 28)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    a = ap.parse_args()
    if any(leg not in LEGS for leg in a.legs.split(",")) or any(k not in KINDS for k in a.kinds.split(",")):
        ap.error(f"--legs: a comma list of {LEGS}; --kinds: of {KINDS}")
    if a.alternate:
        alternate(a)
    elif a.leg:
        run_leg(a)
    else:
        ap.error("give --leg or --alternate")


if __name__ == "__main__":
    main()
