#!/usr/bin/env python3
"""float32 against float16 storage of the RGB step's orient and line_end maps (LineEndPipeline(mode="rgb", rgb_storage=...)), in ONE
process AT THE SAME ADDRESSES (placement=None; the method of scripts/time_gray_float16.py): both pipelines of a workload write one
pyramid buffer, the float16 maps alias the START of the float32 pipeline's orient and line_end allocations, both read bench.py's
seeded frames; timing windows alternate between the three steps

    a   the float32 step
    b   a + a conversion of orient and line_end to preallocated float16 tensors on the same stream (what half-size maps cost today)
    c   the float16 step

and, with silent_set_profiling's events around the chain launch alone, between the chain kernels of a and c.

    python scripts/time_rgb_float16.py [config3 reference_layout ...]   [CALLS=5] [STEPS=20]

Prints one JSON line: per workload min / median / max ms of the windows of a, b, c and of the chain launch alone, whether every window
of c lies below every window of b, c against a (and a's own window spread), and the bytes the chain kernel moves per frame by the model
of DESIGN.md section 4.2 (pyramid read once, every kept map written once)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from pysilent_amd import distributed as D

names = sys.argv[1:] or ["config3", "reference_layout"]
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


def stats(v):
    return {"min": round(float(np.min(v)), 4), "median": round(float(np.median(v)), 4), "max": round(float(np.max(v)), 4)}


def chain_bytes(pipe, color_bytes):
    """The chain kernel per frame: 12 B/px pyramid read, orient (if kept) and line_end written, and the float32 value map where
    it is written -- the kept one, or the one the float16 call with selection keeps in the context workspace for its tail."""
    colour = (2 if pipe.orient_map else 1) * color_bytes
    value = 4 if pipe._value_written else 0
    return {"read": 12 * pipe.frame_px, "colour_maps_written": colour * pipe.frame_px,
            "value_map_written": value * pipe.frame_px, "value_map_in_workspace": bool(value and not pipe.value_map),
            "written": (colour + value) * pipe.frame_px, "total": (12 + colour + value) * pipe.frame_px}


def kernel_ms(pipe, frames, n):
    out = []
    pipe.set_profiling(1)
    for _ in range(n):
        pipe.step(frames)
        torch.cuda.synchronize()
        out.append(pipe.profiled_kernel()[0])
    pipe.set_profiling(0)
    return out


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    pipes = {st: bench.make_pipeline(wl, B, 0, None, rgb_storage=st) for st in ("float32", "float16")}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    f32, f16 = pipes["float32"], pipes["float16"]
    maps = f32._alloc_maps()
    f32._adopt_maps(maps)
    half = {"pyr": maps["pyr"], "value": maps["value"]}
    for k in ("orient", "line_end"):
        half[k] = None if maps[k] is None else maps[k].view(torch.float16)[:maps[k].numel()]
        assert half[k] is None or (half[k].data_ptr() == maps[k].data_ptr() and half[k].numel() == getattr(f16, k).numel())
    f16._adopt_maps(half)
    conv = {k: torch.empty(maps[k].numel(), dtype=torch.float16, device=dev) for k in ("orient", "line_end") if maps[k] is not None}

    def step_a():
        f32.step(frames)

    def step_b():
        f32.step(frames)
        for k, dst in conv.items():
            dst.copy_(getattr(f32, k))

    def step_c():
        f16.step(frames)

    fns = {"a_float32": step_a, "b_float32_then_convert": step_b, "c_float16": step_c}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    kern = {"a_float32": [], "c_float16": []}
    for _ in range(calls):
        for k, fn in fns.items():
            for _ in range(3):
                fn()
            ms[k].append(timed(fn, steps))
        kern["a_float32"] += kernel_ms(f32, frames, 3)
        kern["c_float16"] += kernel_ms(f16, frames, 3)
    a, b, c = ms["a_float32"], ms["b_float32_then_convert"], ms["c_float16"]
    model = {"float32": chain_bytes(f32, 12), "float16": chain_bytes(f16, 6)}
    result[name] = {"frames": B, "steps_per_window": steps, "windows": calls,
                    "step_ms": {k: stats(v) for k, v in ms.items()},
                    "chain_launch_ms": {k: stats(v) for k, v in kern.items()},
                    "every_c_below_every_b": bool(max(c) < min(b)),
                    "c_over_a_median": round(float(np.median(c) / np.median(a)), 4),
                    "a_window_spread": round(float((max(a) - min(a)) / np.median(a)), 4),
                    "c_below_a_beyond_its_spread": bool(max(c) < min(a)),
                    "chain_model_bytes_per_frame": model,
                    "bytes_saved_per_step": (model["float32"]["written"] - model["float16"]["written"]) * B,
                    "colour_map_bytes_saved_per_step": (model["float32"]["colour_maps_written"] - model["float16"]["colour_maps_written"]) * B,
                    "library": os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so")}
    del pipes, f32, f16, maps, half, frames, conv
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
