#!/usr/bin/env python3
"""16-bit planar and packed YUV read in place against "convert to float32 frames, then the float32 step" and against P010 for the RGB
step (LineEndPipeline(mode="rgb", rgb_frame_format="yuv420p10" / "yuv422p10msb")), in ONE process AT THE SAME ADDRESSES
(placement=None): all pipelines of a workload ADOPT THE SAME pyramid and map buffers; timing windows alternate between the variants,
device events around each window.  The method of scripts/time_rgb_yuv.py.

    python scripts/time_rgb_yuv16.py [config3 reference_layout ...]   [CALLS=5] [STEPS=20]

ONE picture -- bench.py's seeded frames as 10-bit BT.709 limited-range YUV, chroma the mean of each 2 x 2 block -- in three kinds of
uint16 surfaces: pitched I010 [B, H * 3 / 2, 2048] (the code in the low bits; chroma planes behind the luma rows at half the pitch),
Y210 [B, H, 4096] (the code in the high bits; every chroma row twice, so the picture is the same) and P010 [B, H * 3 / 2, 2048].  Per
workload, min / median / max ms of
    f32                    (a) the float32-frame step on precomputed converted frames: the floor
    convert_f32_<layout>   (b) silent_yuv16_to_rgb_dev into a preallocated buffer + (a): what such a source costs without this path
    i010, y210             (c) the yuv16 step on the surfaces
    p010                   (d) the P010 step on the same picture
    pyramid_*              the pyramid launch alone (run_pyramid) of (a), (c) and (d)
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
from pysilent_amd.util.zoom import p010_planes, yuv16_planes

names = sys.argv[1:] or ["config3", "reference_layout"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
KINDS = {"i010": ("yuv420p10", 2048), "y210": ("yuv422p10msb", 4096)}     # layout -> (rgb_frame_format, surface pitch in elements)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def to_yuv(frames):
    """BGR float32 frames [B, H, W, 3] -> (y [B, H, W], u, v [B, H / 2, W / 2]) 10-bit codes (int32), BT.709 limited range."""
    B, H, W, _ = frames.shape
    kr, kb = .2126, .0722
    b, g, r = frames[..., 0], frames[..., 1], frames[..., 2]
    yl = kr * r + (1 - kr - kb) * g + kb * b
    pool = lambda x: x.reshape(B, H // 2, 2, W // 2, 2).mean((2, 4))
    u, v = pool((b - yl) / (2 * (1 - kb))), pool((r - yl) / (2 * (1 - kr)))
    return ((64 + yl * (876 / 255)).round().clamp(64, 940).to(torch.int32), (512 + u * (896 / 255)).round().clamp(64, 960).to(torch.int32),
            (512 + v * (896 / 255)).round().clamp(64, 960).to(torch.int32))


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    H, W = wl["hw"]
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    y, u, v = to_yuv(frames)
    del frames
    # what lies beside the pixels is 0xA5A5; the low-aligned codes carry zeros above them, the high-aligned ones zeros below
    surf = {"i010": torch.full((B, H * 3 // 2, 2048), 0xA5A5, dtype=torch.uint16, device=dev),
            "y210": torch.full((B, H, 4096), 0xA5A5, dtype=torch.uint16, device=dev),
            "p010": torch.full((B, H * 3 // 2, 2048), 0xA5A5, dtype=torch.uint16, device=dev)}
    planes = {k: yuv16_planes(surf[k], H, W, k) for k in KINDS}
    planes["p010"] = p010_planes(surf["p010"], H, W)
    low, high = (lambda x: x.to(torch.uint16)), (lambda x: (x << 6).to(torch.uint16))
    planes["i010"][0].copy_(low(y))
    planes["i010"][1].copy_(low(u))
    planes["i010"][2].copy_(low(v))
    planes["y210"][0].copy_(high(y))
    planes["y210"][1].copy_(high(u.repeat_interleave(2, 1)))
    planes["y210"][2].copy_(high(v.repeat_interleave(2, 1)))
    planes["p010"][0].copy_(high(y))
    planes["p010"][1].copy_(high(torch.stack([u, v], -1)))
    del y, u, v
    pipes = {"f32": bench.make_pipeline(wl, B, 0, None), "p010": bench.make_pipeline(wl, B, 0, None, rgb_frame_format="p010")}
    for k, (fmt, _) in KINDS.items():
        pipes[k] = bench.make_pipeline(wl, B, 0, None, rgb_frame_format=fmt)
    m, oy, oc = _runtime.p010_coefficients(depth=10)
    converted = _runtime.yuv16_to_rgb(planes["i010"], (H, W), "yuv420p10")
    assert torch.equal(converted, _runtime.yuv16_to_rgb(planes["y210"], (H, W), "yuv422p10msb")) and torch.equal(converted, _runtime.p010_to_rgb(planes["p010"], (H, W), 10))
    scratch = torch.empty_like(converted)
    ctx = _runtime.get_context(0)
    lib = _lib.load()
    structs = {k: _lib.yuv16_ptr(_runtime.yuv16_frames_of(planes[k], (H, W), KINDS[k][0], m, oy, oc)[0]) for k in KINDS}

    def convert(k):
        ctx.check(lib.silent_yuv16_to_rgb_dev(ctx.handle, structs[k], B, H, W, C.c_void_p(scratch.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    maps = {k: v for k, v in pipes["f32"]._alloc_maps().items() if v is not None}
    for p in pipes.values():
        p._adopt_maps(dict(maps))

    def convert_then_step(k):
        convert(k)
        pipes["f32"].step(scratch)

    variants = {"f32": lambda: pipes["f32"].step(converted), "p010": lambda: pipes["p010"].step(planes["p010"]),
                "pyramid_f32": lambda: pipes["f32"].run_pyramid(converted), "pyramid_p010": lambda: pipes["p010"].run_pyramid(planes["p010"])}
    for k in KINDS:
        variants["convert_f32_" + k] = lambda k=k: convert_then_step(k)
        variants[k] = lambda k=k: pipes[k].step(planes[k])
        variants["convert_" + k] = lambda k=k: convert(k)
        variants["pyramid_" + k] = lambda k=k: pipes[k].run_pyramid(planes[k])
    # the variants write the same buffers: their results must be the same bits (the keypoint rows included)
    digests = {}
    for k, fn in variants.items():
        if k in ("convert_i010", "convert_y210"):
            continue
        for mp in (maps.values() if not k.startswith("pyramid_") else [maps["pyr"]]):
            mp.fill_(-7.0)
        fn()
        torch.cuda.synchronize()
        d = [int(mp.view(torch.int32).to(torch.int64).sum().item()) for mp in (maps.values() if not k.startswith("pyramid_") else [maps["pyr"]])]
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
    f32p = pipes["f32"]
    src_bytes = {"i010": H * W * 3, "y210": H * W * 4}
    entry = {
        "frames": B, "steps_per_call": steps, "calls": calls, "surface_pitch_bytes": {k: 2 * KINDS[k][1] for k in KINDS},
        "walk_plans": {k: list(p.plan.walk_plans) for k, p in pipes.items()},
        "launch_summary": {k: pipes[k].launch_summary() for k in KINDS},
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
        "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
        "windows_ms": {k: [round(float(x), 4) for x in v] for k, v in ms.items()},
        "f32_window_spread_ms": round(float(np.max(ms["f32"]) - np.min(ms["f32"])), 4),
        "p010_window_spread_ms": round(float(np.max(ms["p010"]) - np.min(ms["p010"])), 4),
        "model_bytes_per_frame": {"step_f32": f32p.algorithmic_bytes_per_frame(), "step_p010": pipes["p010"].algorithmic_bytes_per_frame(),
                                  "pyramid_f32": f32p.pyramid_bytes_per_frame(), "pyramid_p010": pipes["p010"].pyramid_bytes_per_frame()},
        "model_ratio": {}, "source_device_bytes": {"p010": int(2 * surf["p010"].numel())},
        "outputs_bit_identical": True}
    for k in KINDS:
        p = pipes[k]
        b_bytes = f32p.algorithmic_bytes_per_frame() + src_bytes[k] + 12 * H * W   # (b): the conversion's read and its 12 B/px write, then (a)
        entry[k + "_over_convert_f32"] = round(med[k] / med["convert_f32_" + k], 4)
        entry[k + "_over_f32"] = round(med[k] / med["f32"], 4)
        entry[k + "_over_p010"] = round(med[k] / med["p010"], 4)
        entry["pyramid_%s_over_f32" % k] = round(med["pyramid_" + k] / med["pyramid_f32"], 4)
        entry["pyramid_%s_over_p010" % k] = round(med["pyramid_" + k] / med["pyramid_p010"], 4)
        entry["every_%s_window_below_every_convert_f32_window" % k] = bool(np.max(ms[k]) < np.min(ms["convert_f32_" + k]))
        entry["model_bytes_per_frame"].update({"step_" + k: p.algorithmic_bytes_per_frame(), "step_convert_f32_" + k: b_bytes,
                                               "pyramid_" + k: p.pyramid_bytes_per_frame()})
        entry["model_ratio"].update({k + "_over_convert_f32": round(p.algorithmic_bytes_per_frame() / b_bytes, 4),
                                     k + "_over_f32": round(p.algorithmic_bytes_per_frame() / f32p.algorithmic_bytes_per_frame(), 4),
                                     k + "_over_p010": round(p.algorithmic_bytes_per_frame() / pipes["p010"].algorithmic_bytes_per_frame(), 4),
                                     "pyramid_%s_over_f32" % k: round(p.pyramid_bytes_per_frame() / f32p.pyramid_bytes_per_frame(), 4)})
        entry["source_device_bytes"].update({k: int(2 * surf[k].numel()), "convert_f32_" + k: int(2 * surf[k].numel() + scratch.numel() * 4)})
    result[name] = entry
    for p in pipes.values():
        p.close()
    del pipes, maps, surf, planes, converted, scratch, variants, structs
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
