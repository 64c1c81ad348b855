#!/usr/bin/env python3
"""P010 decoder surfaces read in place against "convert to float32 frames, then the float32 step" for the RGB step
(LineEndPipeline(mode="rgb", rgb_frame_format="p010")), in ONE process AT THE SAME ADDRESSES (placement=None; the placement of the
maps moves a step by up to 25 %, profiles/r06/placement.md): all pipelines of a workload ADOPT THE SAME pyramid and map buffers;
timing windows alternate between the variants, device events around each window.  The method of scripts/time_rgb_nv12.py.

    python scripts/time_rgb_p010.py [config3 reference_layout ...]   [CALLS=5] [STEPS=20]

The surfaces are [B, H * 3 / 2, 2048] uint16 (luma rows, chroma rows directly below, 4096-byte pitch) carrying bench.py's seeded frames
as BT.709 limited-range 10-bit codes in the high bits (chroma: the mean of each 2 x 2 block); the NV12 surfaces [B, H * 3 / 2, 2048]
uint8 carry the same picture in 8 bits.  Per workload, min / median / max ms of
    f32             (a) the float32-frame step on precomputed converted frames (silent_p010_to_rgb of the surfaces): the floor
    convert_f32     (b) silent_p010_to_rgb_dev into a preallocated buffer + (a): what a 10-bit source cost before
    p010            (c) the P010 step on the surfaces
    nv12            the NV12 step on the 8-bit surfaces of the same picture (other values: not part of the bit comparison)
    pyramid_*       the pyramid launch alone (run_pyramid) of (a), (c) and the NV12 step
beside the byte model of each ratio.  Prints one JSON line."""
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
from pysilent_amd.util.zoom import nv12_planes, p010_planes

names = sys.argv[1:] or ["config3", "reference_layout"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
PITCH = 2048            # elements of a surface row: 4096 bytes (P010), 2048 bytes (NV12)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def to_yuv(frames):
    """BGR float32 frames [B, H, W, 3] on the 0 .. 255 scale -> (Y', U', V') BT.709, chroma pooled over 2 x 2 blocks."""
    B, H, W, _ = frames.shape
    kr, kb = .2126, .0722
    b, g, r = frames[..., 0], frames[..., 1], frames[..., 2]
    yl = kr * r + (1 - kr - kb) * g + kb * b
    pool = lambda x: x.reshape(B, H // 2, 2, W // 2, 2).mean((2, 4))
    return yl, pool((b - yl) / (2 * (1 - kb))), pool((r - yl) / (2 * (1 - kr)))


def surfaces(frames, depth):
    """Limited-range surfaces [B, H * 3 / 2, PITCH] of ``depth`` bits: uint8 for 8, uint16 with the code in the high bits otherwise
    (written as int16 bit patterns and viewed as uint16).  What lies beside the pixels is 0xA5 bytes."""
    B, H, W, _ = frames.shape
    yl, u, v = to_yuv(frames)
    s = 2 ** (depth - 8)
    yc = (16 * s + yl * (219 * s / 255)).round().clamp(16 * s, 235 * s).to(torch.int32)
    cc = torch.stack([(128 * s + u * (224 * s / 255)).round().clamp(16 * s, 240 * s), (128 * s + v * (224 * s / 255)).round().clamp(16 * s, 240 * s)], -1).to(torch.int32)
    if depth == 8:
        surf = torch.full((B, H * 3 // 2, PITCH), 0xA5, dtype=torch.uint8, device=frames.device)
        y, uv = nv12_planes(surf, H, W)
        y.copy_(yc.to(torch.uint8))
        uv.copy_(cc.to(torch.uint8))
        return surf
    raw = torch.full((B, H * 3 // 2, PITCH), 0xA5A5 - 0x10000, dtype=torch.int16, device=frames.device)
    y, uv = raw[:, :H, :W], raw[:, H:H + H // 2, :W].unflatten(2, (W // 2, 2))
    y.copy_((yc << (16 - depth)).to(torch.int16))              # (the low 16 bits: the cast wraps)
    uv.copy_((cc << (16 - depth)).to(torch.int16))
    return raw.view(torch.uint16)


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    H, W = wl["hw"]
    pipes = {"f32": bench.make_pipeline(wl, B, 0, None), "p010": bench.make_pipeline(wl, B, 0, None, rgb_frame_format="p010"),
             "nv12": bench.make_pipeline(wl, B, 0, None, rgb_frame_format="nv12")}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    surf, surf8 = surfaces(frames, 10), surfaces(frames, 8)
    del frames
    planes, planes8 = p010_planes(surf, H, W), nv12_planes(surf8, H, W)
    m, oy, oc = _runtime.p010_coefficients(depth=10)
    converted = _runtime.p010_to_rgb(planes, (H, W))
    scratch = torch.empty_like(converted)
    ctx = _runtime.get_context(0)
    lib = _lib.load()
    struct = _lib.p010_ptr(_runtime.p010_frames_of(planes, (H, W), m, oy, oc, 10)[0])

    def convert():
        ctx.check(lib.silent_p010_to_rgb_dev(ctx.handle, struct, B, H, W, C.c_void_p(scratch.data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    maps = {k: v for k, v in pipes["f32"]._alloc_maps().items() if v is not None}
    for p in pipes.values():
        p._adopt_maps(dict(maps))

    def convert_then_step():
        convert()
        pipes["f32"].step(scratch)

    variants = {"f32": lambda: pipes["f32"].step(converted), "convert_f32": convert_then_step, "p010": lambda: pipes["p010"].step(planes),
                "nv12": lambda: pipes["nv12"].step(planes8), "convert": convert,
                "pyramid_f32": lambda: pipes["f32"].run_pyramid(converted), "pyramid_p010": lambda: pipes["p010"].run_pyramid(planes),
                "pyramid_nv12": lambda: pipes["nv12"].run_pyramid(planes8)}
    # the variants of the 10-bit source write the same buffers: their results must be the same bits (the keypoint rows included)
    digests = {}
    for k, fn in variants.items():
        if k == "convert":
            continue
        for mp in (maps.values() if not k.startswith("pyramid_") else [maps["pyr"]]):
            mp.fill_(-7.0)
        fn()
        torch.cuda.synchronize()
        d = [int(mp.view(torch.int32).to(torch.int64).sum().item()) for mp in (maps.values() if not k.startswith("pyramid_") else [maps["pyr"]])]
        if not k.startswith("pyramid_"):
            p = pipes[k if k in ("p010", "nv12") else "f32"]
            d += [int(p.kp_counts.sum().item()), int(p.kp_idx[0, :int(min(p.kp_counts[0].item(), p.kp_cap))].sum().item())]
        digests[k] = d
    assert digests["f32"] == digests["p010"] == digests["convert_f32"], digests
    assert digests["pyramid_f32"] == digests["pyramid_p010"] == digests["f32"][:1], digests
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
    f32p, pp, nvp = pipes["f32"], pipes["p010"], pipes["nv12"]
    before = f32p.algorithmic_bytes_per_frame() + 3 * H * W + 12 * H * W
    result[name] = {
        "frames": B, "steps_per_call": steps, "calls": calls, "surface_pitch_bytes": {"p010": 2 * PITCH, "nv12": PITCH},
        "walk_plans": {k: list(p.plan.walk_plans) for k, p in pipes.items()},
        "launch_summary": pp.launch_summary(),
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
        "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
        "windows_ms": {k: [round(float(x), 4) for x in v] for k, v in ms.items()},
        "p010_over_convert_f32": round(med["p010"] / med["convert_f32"], 4),
        "p010_over_f32": round(med["p010"] / med["f32"], 4),
        "p010_over_nv12": round(med["p010"] / med["nv12"], 4),
        "pyramid_p010_over_f32": round(med["pyramid_p010"] / med["pyramid_f32"], 4),
        "pyramid_p010_over_nv12": round(med["pyramid_p010"] / med["pyramid_nv12"], 4),
        "every_p010_window_below_every_convert_f32_window": bool(np.max(ms["p010"]) < np.min(ms["convert_f32"])),
        "p010_below_convert_f32_window_by_window": [bool(a < b) for a, b in zip(ms["p010"], ms["convert_f32"])],
        "f32_window_spread_ms": round(float(np.max(ms["f32"]) - np.min(ms["f32"])), 4),
        # bytes per frame: the step and the pyramid launch of each variant; (b) adds the conversion's read of 3 B/px and its write of
        # 12 B/px to (a), which then reads the 12 B/px back
        "model_bytes_per_frame": {"step_f32": f32p.algorithmic_bytes_per_frame(), "step_p010": pp.algorithmic_bytes_per_frame(),
                                  "step_nv12": nvp.algorithmic_bytes_per_frame(), "step_convert_f32": before,
                                  "pyramid_f32": f32p.pyramid_bytes_per_frame(), "pyramid_p010": pp.pyramid_bytes_per_frame(),
                                  "pyramid_nv12": nvp.pyramid_bytes_per_frame()},
        "model_ratio": {"p010_over_convert_f32": round(pp.algorithmic_bytes_per_frame() / before, 4),
                        "p010_over_f32": round(pp.algorithmic_bytes_per_frame() / f32p.algorithmic_bytes_per_frame(), 4),
                        "p010_over_nv12": round(pp.algorithmic_bytes_per_frame() / nvp.algorithmic_bytes_per_frame(), 4),
                        "pyramid_p010_over_f32": round(pp.pyramid_bytes_per_frame() / f32p.pyramid_bytes_per_frame(), 4)},
        "source_device_bytes": {"p010": int(surf.numel() * 2), "convert_f32": int(surf.numel() * 2 + scratch.numel() * 4)},
        "outputs_bit_identical": True}
    for p in pipes.values():
        p.close()
    del pipes, maps, surf, surf8, planes, planes8, converted, scratch, variants
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
