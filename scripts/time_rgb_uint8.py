#!/usr/bin/env python3
"""float32 colour frames against packed uint8 colour frames for the RGB step (LineEndPipeline(mode="rgb", rgb_frame_dtype=...)), in
ONE process AT THE SAME ADDRESSES (placement=None; the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md):
both pipelines of a workload ADOPT THE SAME pyramid and map buffers, the float32 pipeline reads bench.py's seeded frames and the
uint8 pipeline their uint8 originals (the seeded frames are uint8 values held as float32); timing windows alternate between the
variants, device events around each window.

    python scripts/time_rgb_uint8.py [config3 reference_layout ...]   [CALLS=5] [STEPS=20] [HOST_CALLS=6]

Per workload, min / median / max ms of
    float32        (a) the float32-frame step on resident float32 frames
    cast_float32   (b) the widening cast of the resident uint8 frames (silent_cast_interleave_dev) + (a): what a uint8 source costs
                       without rgb_frame_dtype="uint8"
    uint8          (c) the uint8-frame step on the resident uint8 frames
    pyramid_*      the pyramid launch alone (run_pyramid) of (a) and (c)
beside the byte model (frame read + pyramid written by the walk launch; algorithmic_bytes_per_frame for the step).  Separately:
step_host frames / s from pinned uint8 host frames on both pipelines, and the device bytes of the ingest ring each of them holds.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from pysilent_amd import _runtime
from pysilent_amd import distributed as D

names = sys.argv[1:] or ["config3", "reference_layout"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
host_calls = int(os.environ.get("HOST_CALLS", "6"))
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


def host_rate(pipe, src, B):
    """step_host frames / s: two batches to fill the ring, then ``host_calls`` batches timed on the host clock."""
    for _ in range(2):
        pipe.step_host(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(host_calls):
        pipe.step_host(src)
    pipe.wait()
    torch.cuda.synchronize()
    return B * host_calls / (time.perf_counter() - t0)


def ring_bytes(pipe):
    slots = pipe._ingest[torch.uint8]["slots"]
    return int(sum(t.numel() * t.element_size() for s in slots for t in (s["raw"], s["f32"]) if t is not None))


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    pipes = {fd: bench.make_pipeline(wl, B, 0, None, rgb_frame_dtype=fd) for fd in ("float32", "uint8")}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    u8 = frames.to(torch.uint8)
    assert torch.equal(u8.to(torch.float32), frames), "bench.py's seeded frames are uint8 values"
    cast_buf = torch.empty_like(frames)
    maps = {k: v for k, v in pipes["float32"]._alloc_maps().items() if v is not None}
    for p in pipes.values():
        p._adopt_maps(dict(maps))
    n_px = frames.numel() // 3

    def cast_then_step():
        _runtime.cast_interleave(u8, cast_buf, 3, 0, 3, 3, 0, n_px)
        pipes["float32"].step(cast_buf)

    variants = {"float32": lambda: pipes["float32"].step(frames), "cast_float32": cast_then_step, "uint8": lambda: pipes["uint8"].step(u8),
                "pyramid_float32": lambda: pipes["float32"].run_pyramid(frames), "pyramid_uint8": lambda: pipes["uint8"].run_pyramid(u8)}
    # the variants write the same buffers: their results must be the same bits (the keypoint rows included)
    digests = {}
    for k, fn in variants.items():
        if k.startswith("pyramid_"):
            maps["pyr"].fill_(-7.0)
        else:
            for m in maps.values():
                m.fill_(-7.0)
        fn()
        torch.cuda.synchronize()
        d = [int(m.view(torch.int32).to(torch.int64).sum().item()) for m in (maps.values() if not k.startswith("pyramid_") else [maps["pyr"]])]
        if not k.startswith("pyramid_"):
            p = pipes["uint8" if k == "uint8" else "float32"]
            d += [int(p.kp_counts.sum().item()), int(p.kp_idx[0, :int(min(p.kp_counts[0].item(), p.kp_cap))].sum().item())]
        digests[k] = d
    assert digests["float32"] == digests["uint8"] == digests["cast_float32"], digests
    assert digests["pyramid_float32"] == digests["pyramid_uint8"] == digests["float32"][:1], digests
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(calls):
        for k, fn in variants.items():
            for _ in range(3):
                fn()
            ms[k].append(timed(fn, steps))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread_a = float(np.max(ms["float32"]) - np.min(ms["float32"]))
    model = {k: {"frame_read": p._frame_bytes * p.frame_shape[0] * p.frame_shape[1] * 3, "walk_launch": p.pyramid_bytes_per_frame(),
                 "step": p.algorithmic_bytes_per_frame()} for k, p in pipes.items()}
    # ingest: pinned uint8 host frames through step_host of both pipelines
    host_pinned = u8.cpu().pin_memory()
    ingest = {}
    for k, p in pipes.items():
        ingest[k] = {"pinned_frames_per_s": round(host_rate(p, host_pinned, B), 1), "ring_device_bytes": ring_bytes(p)}
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls,
                    "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
                    "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
                    "windows_ms": {k: [round(float(x), 4) for x in v] for k, v in ms.items()},
                    "uint8_over_float32": round(med["uint8"] / med["float32"], 4),
                    "uint8_over_cast_float32": round(med["uint8"] / med["cast_float32"], 4),
                    "pyramid_uint8_over_float32": round(med["pyramid_uint8"] / med["pyramid_float32"], 4),
                    "every_uint8_window_below_every_cast_float32_window": bool(np.max(ms["uint8"]) < np.min(ms["cast_float32"])),
                    "uint8_minus_float32_ms": round(med["uint8"] - med["float32"], 4), "float32_window_spread_ms": round(spread_a, 4),
                    "uint8_exceeds_float32_by_more_than_its_spread": bool(med["uint8"] - med["float32"] > spread_a),
                    "model_bytes_per_frame": model,
                    "model_byte_ratio": {k: round(model["uint8"][k] / model["float32"][k], 4) for k in model["float32"]},
                    "step_host_uint8_frames": ingest, "host_calls": host_calls,
                    "resident_frame_bytes": {"float32": int(frames.numel() * 4), "uint8": int(u8.numel())},
                    "outputs_bit_identical": True,
                    "library": os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so"),
                    "walk_plans": {k: list(p.plan.walk_plans) for k, p in pipes.items()}}
    for p in pipes.values():
        p.close()
    del pipes, maps, frames, u8, cast_buf, variants, host_pinned
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
