#!/usr/bin/env python3
"""Raw 8-bit Bayer mosaics read in place against "demosaic to float32 frames, then the float32 step" for the RGB step
(LineEndPipeline(mode="rgb", rgb_frame_format="bayer_rggb")), in ONE process AT THE SAME ADDRESSES (placement=None): all pipelines of a
workload ADOPT THE SAME pyramid and map buffers; timing windows alternate between the variants, device events around each window.  The
method of scripts/time_rgb_nv12.py.

    python scripts/time_rgb_bayer.py [config3 reference_layout ...]   [CALLS=5] [STEPS=20]

ONE picture -- bench.py's seeded frames, rounded to bytes and sampled as an RGGB sensor would (the red byte of a pixel at an even row
and column, ...) -- as a pitched mosaic [B, H, 2048] (what lies beside the pixels is 0xA5).  Per workload, min / median / max ms of
    f32                    (a) the float32-frame step on precomputed converted frames: the floor
    convert_f32            (b) silent_bayer_to_rgb_dev into a preallocated buffer + (a): what a Bayer source costs without this path
    bayer                  (c) the Bayer step on the mosaic
    rgb8                   the packed rgb_frame_dtype="uint8" step on the picture the mosaic was sampled from (3 B/px; other bits: a
                           sensor does not deliver it)
    pyramid_*              the pyramid launch alone (run_pyramid) of (a), (c) and rgb8; convert: the conversion launch alone;
                           pyramid_*_unit_region: the same launch under PYRAMID knob 2 (unit + region kernels: nine loads a tap)
beside the byte model of each ratio and the device memory a source holds.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from pysilent_amd import _lib, _runtime
from pysilent_amd import distributed as D

names = sys.argv[1:] or ["config3", "reference_layout"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
FMT, PITCH = "bayer_rggb", 2048


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def to_mosaic(bgr8):
    """uint8 BGR frames [B, H, W, 3] -> the RGGB mosaic [B, H, W] a sensor records of them."""
    m = bgr8[..., 1].clone()                           # green everywhere ...
    m[:, 0::2, 0::2] = bgr8[:, 0::2, 0::2, 2]          # ... red at (even, even)
    m[:, 1::2, 1::2] = bgr8[:, 1::2, 1::2, 0]          # ... blue at (odd, odd)
    return m


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    H, W = wl["hw"]
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    bgr8 = frames.round().clamp(0, 255).to(torch.uint8).contiguous()
    del frames
    surf = torch.full((B, H, PITCH), 0xA5, dtype=torch.uint8, device=dev)
    mosaic = surf[:, :, :W]
    mosaic.copy_(to_mosaic(bgr8))
    pipes = {"f32": bench.make_pipeline(wl, B, 0, None), "bayer": bench.make_pipeline(wl, B, 0, None, rgb_frame_format=FMT),
             "rgb8": bench.make_pipeline(wl, B, 0, None, rgb_frame_dtype="uint8")}
    converted = _runtime.bayer_to_rgb(mosaic, (H, W), FMT)
    scratch = torch.empty_like(converted)
    ctx = _runtime.get_context(0)
    lib = _lib.load()
    struct = _lib.bayer_ptr(_runtime.bayer_frames_of(mosaic, (H, W), FMT)[0])

    def convert():
        ctx.check(lib.silent_bayer_to_rgb_dev(ctx.handle, struct, B, H, W, C.c_void_p(scratch.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    maps = {k: v for k, v in pipes["f32"]._alloc_maps().items() if v is not None}
    for p in pipes.values():
        p._adopt_maps(dict(maps))

    def convert_then_step():
        convert()
        pipes["f32"].step(scratch)

    variants = {"f32": lambda: pipes["f32"].step(converted), "convert_f32": convert_then_step, "bayer": lambda: pipes["bayer"].step(mosaic),
                "rgb8": lambda: pipes["rgb8"].step(bgr8), "convert": convert, "pyramid_f32": lambda: pipes["f32"].run_pyramid(converted),
                "pyramid_bayer": lambda: pipes["bayer"].run_pyramid(mosaic), "pyramid_rgb8": lambda: pipes["rgb8"].run_pyramid(bgr8)}
    def unit_region(fn):
        """fn under PYRAMID knob 2: the unit + region kernels instead of the walk."""
        def run():
            ctx.set_tuning(_lib.TUNE_PYRAMID, 2)
            try:
                fn()
            finally:
                ctx.set_tuning(_lib.TUNE_PYRAMID, 0)
        return run

    variants["pyramid_f32_unit_region"] = unit_region(variants["pyramid_f32"])
    variants["pyramid_bayer_unit_region"] = unit_region(variants["pyramid_bayer"])
    # the variants of the SAME picture write the same buffers: their results must be the same bits (the keypoint rows included)
    digests = {}
    for k in ("f32", "convert_f32", "bayer", "pyramid_f32", "pyramid_bayer", "pyramid_f32_unit_region", "pyramid_bayer_unit_region"):
        targets = list(maps.values()) if not k.startswith("pyramid_") else [maps["pyr"]]
        for mp in targets:
            mp.fill_(-7.0)
        variants[k]()
        torch.cuda.synchronize()
        d = [int(mp.view(torch.int32).to(torch.int64).sum().item()) for mp in targets]
        if not k.startswith("pyramid_"):
            p = pipes[k if k in pipes else "f32"]
            d += [int(p.kp_counts.sum().item()), int(p.kp_idx[0, :int(min(p.kp_counts[0].item(), p.kp_cap))].sum().item())]
        digests[k] = d
    assert all(digests[k] == digests["f32"] for k in digests if not k.startswith("pyramid_")), digests
    assert all(digests[k] == digests["f32"][:1] for k in digests if k.startswith("pyramid_")), digests
    assert torch.equal(scratch, converted)
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
    f32p, bp = pipes["f32"], pipes["bayer"]
    b_bytes = f32p.algorithmic_bytes_per_frame() + H * W + 12 * H * W      # (b): the conversion's read and its 12 B/px write, then (a)
    result[name] = {
        "frames": B, "steps_per_call": steps, "calls": calls, "format": FMT, "mosaic_pitch_bytes": PITCH,
        "walk_plans": {k: list(p.plan.walk_plans) for k, p in pipes.items()},
        "launch_summary": bp.launch_summary(),
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
        "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
        "windows_ms": {k: [round(float(x), 4) for x in v] for k, v in ms.items()},
        "f32_window_spread_ms": round(float(np.max(ms["f32"]) - np.min(ms["f32"])), 4),
        "bayer_over_convert_f32": round(med["bayer"] / med["convert_f32"], 4),
        "bayer_over_f32": round(med["bayer"] / med["f32"], 4),
        "bayer_over_rgb8": round(med["bayer"] / med["rgb8"], 4),
        "pyramid_bayer_over_f32": round(med["pyramid_bayer"] / med["pyramid_f32"], 4),
        "pyramid_bayer_over_rgb8": round(med["pyramid_bayer"] / med["pyramid_rgb8"], 4),
        "pyramid_unit_region_bayer_over_f32": round(med["pyramid_bayer_unit_region"] / med["pyramid_f32_unit_region"], 4),
        "every_bayer_window_below_every_convert_f32_window": bool(np.max(ms["bayer"]) < np.min(ms["convert_f32"])),
        "model_bytes_per_frame": {"step_f32": f32p.algorithmic_bytes_per_frame(), "step_bayer": bp.algorithmic_bytes_per_frame(),
                                  "step_convert_f32": b_bytes, "step_rgb8": pipes["rgb8"].algorithmic_bytes_per_frame(),
                                  "pyramid_f32": f32p.pyramid_bytes_per_frame(), "pyramid_bayer": bp.pyramid_bytes_per_frame()},
        "model_ratio": {"bayer_over_convert_f32": round(bp.algorithmic_bytes_per_frame() / b_bytes, 4),
                        "bayer_over_f32": round(bp.algorithmic_bytes_per_frame() / f32p.algorithmic_bytes_per_frame(), 4),
                        "pyramid_bayer_over_f32": round(bp.pyramid_bytes_per_frame() / f32p.pyramid_bytes_per_frame(), 4)},
        "source_device_bytes": {"mosaic_pixels": B * H * W, "mosaic_surfaces": int(surf.numel()), "float32_copy": int(scratch.numel() * 4),
                                "convert_f32": int(surf.numel() + scratch.numel() * 4), "rgb8": int(bgr8.numel())},
        "outputs_bit_identical": True}
    for p in pipes.values():
        p.close()
    del pipes, maps, surf, mosaic, converted, scratch, variants, struct, bgr8
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
