#!/usr/bin/env python3
"""float32 against float16 storage of the gray step's CS and end maps (LineEndPipeline(mode="gray", storage=...)), in ONE process
AT THE SAME ADDRESSES (placement=None; the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md): both
pipelines of a workload write one pyramid buffer, the float16 maps alias the START of the float32 pipeline's CS and end
allocations, both read bench.py's seeded frames; timing windows alternate between them.

    python scripts/time_gray_float16.py [config2 config5 ...]   [CALLS=5] [STEPS=20]

Prints one JSON line: per workload min / median / max ms per step of `float32` and `float16`, their ratio, and the byte ratio of
DESIGN.md section 4.2's per-pixel model (level 0: 4 read + 4 pyramid + CS + K end; other levels: 4 pyramid write + 4 read + CS + K
end) that the measured ratio is held against."""
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


def model_bytes(pipe, map_bytes):
    """DESIGN 4.2's bytes per frame: gray_stream_kernel (frame read, pyramid of every level, CS + end of level 0) and
    gray_line_end_kernel (pyramid read, CS + end of the other levels)."""
    K = pipe.n_orient
    px0 = pipe.extents[0][0] * pipe.extents[0][1]
    rest = pipe.frame_px - px0
    stream = px0 * (4 + 4 + map_bytes * (1 + K)) + rest * 4
    line_end = rest * (4 + map_bytes * (1 + K))
    return {"gray_stream_kernel": stream, "gray_line_end_kernel": line_end, "step": stream + line_end}


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    pipes = {st: bench.make_pipeline(wl, B, 0, None, storage=st) for st in ("float32", "float16")}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    maps = pipes["float32"]._alloc_maps()
    pipes["float32"]._adopt_maps(maps)
    half = {"pyr": maps["pyr"]}
    for k in ("cs", "end"):
        half[k] = maps[k].view(torch.float16)[:maps[k].numel()]
        assert half[k].data_ptr() == maps[k].data_ptr() and half[k].numel() == pipes["float16"].__dict__[k].numel()
    pipes["float16"]._adopt_maps(half)
    for p in pipes.values():
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
    model = {k: model_bytes(pipes[k], 2 if k == "float16" else 4) for k in pipes}
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls,
                    "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
                    "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
                    "float16_over_float32": round(med["float16"] / med["float32"], 4),
                    "model_bytes_per_frame": model,
                    "model_byte_ratio": {k: round(model["float16"][k] / model["float32"][k], 4) for k in model["float32"]},
                    "library": os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so"),
                    "streamable": {k: p.plan.streamable for k, p in pipes.items()}}
    del pipes, maps, half, frames
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
