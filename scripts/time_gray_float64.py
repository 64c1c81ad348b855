#!/usr/bin/env python3
"""Float32 against float64 accumulation of the gray step (LineEndPipeline(mode="gray", accumulation=...)), in ONE process ON THE
SAME BUFFERS (placement=None; the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md): both pipelines of a
workload adopt one set of maps and read bench.py's seeded frames; timing windows alternate between them.

    python scripts/time_gray_float64.py [config2 config5 ...]   [CALLS=5] [STEPS=20]

Prints one JSON line: per workload the median (and min) ms per step of `float32` and `float64`, and their ratio."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from pysilent_amd import distributed as D

names = sys.argv[1:] or ["config2", "config5"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    pipes = {acc: bench.make_pipeline(wl, B, 0, None, accumulation=acc) for acc in ("float32", "float64")}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    maps = pipes["float32"]._alloc_maps()
    for p in pipes.values():
        p._adopt_maps(maps)
        for _ in range(10):
            p.step(frames)
    torch.cuda.synchronize()
    ms = {k: [] for k in pipes}
    for _ in range(calls):
        for k, p in pipes.items():
            for _ in range(3):
                p.step(frames)
            ms[k].append(timed(lambda: p.step(frames), steps))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls,
                    "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
                    "float64_over_float32": round(med["float64"] / med["float32"], 4),
                    "streamable": {k: p.plan.streamable for k, p in pipes.items()}}
    del pipes, maps, frames
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
