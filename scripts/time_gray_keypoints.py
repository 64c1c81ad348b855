#!/usr/bin/env python3
"""Maps-only gray step against the keypoint step (LineEndPipeline(mode="gray", keypoints=True): silent_gray_keypoints_dev), in ONE
process ON THE SAME BUFFERS (the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md): every pipeline of a
workload adopts one set of maps and reads bench.py's seeded frames; timing windows alternate between them.

    python scripts/time_gray_keypoints.py [config2 config5 ...]   [CALLS=5] [STEPS=20]

Prints one JSON line: per workload the median (and min) ms per step of `maps` (keypoints=False), `kp_selection`
(selection=True, no value / peak-value map: the sparse tail) and `kp_plain` (selection=False: a-11 on the value map), their ratios
to `maps`, and sparse_tail_stats of the selection step."""
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
    variants = {"maps": {}, "kp_selection": {"keypoints": True, "selection": True}, "kp_plain": {"keypoints": True, "selection": False}}
    pipes = {k: bench.make_pipeline(wl, B, 0, None, **kw) for k, kw in variants.items()}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    maps = pipes["maps"]._alloc_maps()
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
    pipes["kp_selection"].step(frames)
    torch.cuda.synchronize()
    stats = pipes["kp_selection"].sparse_tail_stats()
    counts = pipes["kp_selection"].kp_counts.cpu().numpy()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls,
                    "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
                    "ratio_to_maps": {k: round(med[k] / med["maps"], 4) for k in med if k != "maps"},
                    "keypoints_per_frame_selection": int(counts.mean()),
                    "sparse_tail_stats": stats}
    del pipes, maps, frames
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
