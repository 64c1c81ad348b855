#!/usr/bin/env python3
"""Strided uint8 colour views against "pack, then the packed uint8 step" for the RGB step (LineEndPipeline(mode="rgb",
rgb_frame_dtype="uint8", rgb_frame_layout=...)), in ONE process AT THE SAME ADDRESSES (placement=None; the placement of the maps
moves a step by up to 25 %, profiles/r06/placement.md): both pipelines of a workload ADOPT THE SAME pyramid and map buffers; timing
windows alternate between the variants, device events around each window.

    python scripts/time_rgb_strided.py [config3 reference_layout ...]   [CALLS=5] [STEPS=20]

Views of bench.py's seeded frames (as uint8):
    bgra      [B, H, W, 4][..., :3]: 3 of 4 bytes
    pitched   BGR rows padded to a multiple of 256 bytes
    region    the centre [H, W] of frames [2 H, 2 W] (a 1080p window of 4K frames)
Per workload and view, min / median / max ms of
    packed        (a) the packed uint8 step on a precomputed packed copy of the view: the floor
    pack_packed   (b) packed.copy_(view) into a preallocated buffer + (a): what such a source costs without rgb_frame_layout="strided"
    strided       (c) the strided step on the view
    pyramid_*     the pyramid launch alone (run_pyramid) of (a) and (c)
beside the byte model (bytes of the view's rows the walk launch passes over, against the packed frame's), and the device memory the
source holds for (b) and (c).  Prints one JSON line."""
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


def make_view(kind, u8):
    """(parent, view) carrying the packed batch ``u8`` [B, H, W, 3]; what lies between the pixels is 0xA5."""
    B, H, W, _ = u8.shape
    if kind == "bgra":
        parent = torch.full((B, H, W, 4), 0xA5, dtype=torch.uint8, device=dev)
        view = parent[..., :3]
    elif kind == "pitched":
        pitch = (3 * W + 255) // 256 * 256
        parent = torch.full((B * H * pitch,), 0xA5, dtype=torch.uint8, device=dev)
        view = torch.as_strided(parent, (B, H, W, 3), (H * pitch, pitch, 3, 1))
    else:
        parent = torch.full((B, 2 * H, 2 * W, 3), 0xA5, dtype=torch.uint8, device=dev)
        view = parent[:, H // 2:H // 2 + H, W // 2:W // 2 + W]
    view.copy_(u8)
    assert not view.is_contiguous() and torch.equal(view.contiguous(), u8)
    return parent, view


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    pipes = {"packed": bench.make_pipeline(wl, B, 0, None, rgb_frame_dtype="uint8"),
             "strided": bench.make_pipeline(wl, B, 0, None, rgb_frame_dtype="uint8", rgb_frame_layout="strided")}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    u8 = frames.to(torch.uint8)
    assert torch.equal(u8.to(torch.float32), frames), "bench.py's seeded frames are uint8 values"
    del frames
    maps = {k: v for k, v in pipes["packed"]._alloc_maps().items() if v is not None}
    for p in pipes.values():
        p._adopt_maps(dict(maps))
    H, W = wl["hw"]
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls, "views": {},
                    "walk_plans": {k: list(p.plan.walk_plans) for k, p in pipes.items()},
                    "launch_summary": pipes["strided"].launch_summary(),
                    "library": os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so")}
    for kind in ("bgra", "pitched", "region"):
        parent, view = make_view(kind, u8)
        packed = torch.empty_like(u8)
        packed.copy_(view)

        def pack_then_step():
            packed.copy_(view)
            pipes["packed"].step(packed)

        variants = {"packed": lambda: pipes["packed"].step(packed), "pack_packed": pack_then_step, "strided": lambda: pipes["strided"].step(view),
                    "pyramid_packed": lambda: pipes["packed"].run_pyramid(packed), "pyramid_strided": lambda: pipes["strided"].run_pyramid(view)}
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
                p = pipes["strided" if k == "strided" else "packed"]
                d += [int(p.kp_counts.sum().item()), int(p.kp_idx[0, :int(min(p.kp_counts[0].item(), p.kp_cap))].sum().item())]
            digests[k] = d
        assert digests["packed"] == digests["strided"] == digests["pack_packed"], digests
        assert digests["pyramid_packed"] == digests["pyramid_strided"] == digests["packed"][:1], digests
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
        sb, sr, sp, _ = (int(s) for s in view.stride())
        row_bytes = (W - 1) * sp + 3
        spread_a = float(np.max(ms["packed"]) - np.min(ms["packed"]))
        result[name]["views"][kind] = {
            "strides_bytes": {"frame": sb, "row": sr, "pixel": sp},
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
            "windows_ms": {k: [round(float(x), 4) for x in v] for k, v in ms.items()},
            "strided_over_pack_packed": round(med["strided"] / med["pack_packed"], 4),
            "strided_over_packed": round(med["strided"] / med["packed"], 4),
            "pyramid_strided_over_packed": round(med["pyramid_strided"] / med["pyramid_packed"], 4),
            "every_strided_window_below_every_pack_packed_window": bool(np.max(ms["strided"]) < np.min(ms["pack_packed"])),
            "packed_window_spread_ms": round(spread_a, 4),
            # bytes per frame: the pixel bytes (what the packed launch reads), and the bytes of the view's rows from their first to
            # their last pixel byte (what a launch that passes over whole cache lines of a BGRA or padded row moves)
            "model_bytes_per_frame": {"pixel_bytes": 3 * H * W, "view_row_bytes": H * row_bytes,
                                      "walk_launch_packed": pipes["packed"].pyramid_bytes_per_frame(),
                                      "walk_launch_view_rows": pipes["packed"].pyramid_bytes_per_frame() - 3 * H * W + H * row_bytes,
                                      "step": pipes["packed"].algorithmic_bytes_per_frame()},
            "source_device_bytes": {"strided": int(parent.numel()), "pack_packed": int(parent.numel() + packed.numel())},
            "outputs_bit_identical": True}
        del parent, view, packed, variants
        torch.cuda.empty_cache()
    for p in pipes.values():
        p.close()
    del pipes, maps, u8
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
