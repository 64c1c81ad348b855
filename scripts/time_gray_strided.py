#!/usr/bin/env python3
"""What a STRIDED uint8 source costs the gray step (LineEndPipeline(mode="gray", frame_dtype="uint8", frame_layout="strided")), in ONE
process AT THE SAME ADDRESSES (placement=None; the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md):
every pipeline of a workload ADOPTS THE SAME pyramid, CS and end buffers; timing windows alternate between the variants.

    python scripts/time_gray_strided.py [config2 config5 ...]   [CALLS=5] [STEPS=20]

Layouts (H x W the workload's frame, B its batch):
    nv12_luma   surface[:, :H, :W, None] of a [B, H * 3 / 2, pitch] uint8 surface batch, pitch = W rounded up to the next power of two
                (1920 -> 2048, 3840 -> 4096): the luma plane of a decoder's NV12 output
    bgra        bgra[..., :3] of [B, H, W, 4]: three of every four bytes
    roi         big[:, y0:y0 + H, x0:x0 + W, None] of frames twice as high and wide (1080p inside 4K for config 2), odd y0 and x0
Per layout, min / median / max ms per step of
    packed      (a) the packed uint8 step on a PRECOMPUTED packed copy of the view: the floor
    pack_step   (b) what the source costs without frame_layout="strided": one launch that packs the view into a preallocated
                    second buffer (packed.copy_(view), what .contiguous() launches, without its allocation), then the packed step
    strided     (c) the strided step on the view
and c / b, c / a beside a byte model: DESIGN.md section 4.2's bytes per frame with the frame read counted as the 128-byte lines the
view's pixels touch (a BGRA row touches every line of its 4 B/px; a pitched or windowed row at most one line more than its packed
bytes); (b) adds the same lines read and the packed bytes written before its step.  (b) and (c) write the same buffers and must
leave the same bits.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from pysilent_amd import _runtime
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


def lines_per_frame(view, channels, h, w):
    """128-byte lines of device memory the pixels of ONE frame of the view touch (frame 0; the address as it is)."""
    address, ch, pixel, row, _ = _runtime.frame_view_of(view, channels)
    first = address + np.arange(h, dtype=np.int64) * row
    last = first + (w - 1) * pixel + ch - 1
    if pixel >= 128:
        return int(h * w)
    return int((last // 128 - first // 128 + 1).sum())


def model_bytes(pipe, frame_bytes_per_frame, before=0):
    """DESIGN 4.2's bytes per frame: gray_stream_kernel (frame read, pyramid of every level, CS + end of level 0) and
    gray_line_end_kernel (pyramid read, CS + end of the other levels); before: bytes per frame moved before the step."""
    K = pipe.n_orient
    px0 = pipe.extents[0][0] * pipe.extents[0][1]
    rest = pipe.frame_px - px0
    stream = frame_bytes_per_frame + px0 * (4 + 4 * (1 + K)) + rest * 4
    line_end = rest * (4 + 4 * (1 + K))
    return {"frame_read": frame_bytes_per_frame, "before_the_step": before, "step": stream + line_end + before}


def make_views(B, h, w, gray, colour):
    """name -> (view, channels): the same pixels in three layouts a source delivers."""
    pitch = 1 << (w - 1).bit_length()
    surface = torch.full((B, h * 3 // 2, pitch), 0x80, dtype=torch.uint8, device=dev)
    surface[:, :h, :w] = gray[..., 0]
    bgra = torch.full((B, h, w, 4), 0xFF, dtype=torch.uint8, device=dev)
    bgra[..., :3] = colour
    big = torch.full((B, 2 * h, 2 * w), 0x40, dtype=torch.uint8, device=dev)
    y0, x0 = h // 2 - 9, w // 2 - 3                        # both odd for 1080p and 4K
    big[:, y0:y0 + h, x0:x0 + w] = gray[..., 0]
    return {"nv12_luma": (surface[:, :h, :w, None], 1), "bgra": (bgra[..., :3], 3), "roi": (big[:, y0:y0 + h, x0:x0 + w, None], 1)}


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    assert wl["mode"] == "gray", name
    B = wl["frames"]
    h, w = wl["hw"]
    host = np.stack([D.synthetic_frame(gi, h, w, 3) for gi in D.shard_frame_indices(B, 0, 1)]).astype(np.uint8)
    colour = torch.from_numpy(host).to(dev)
    gray = colour[..., 1:2].contiguous()
    del host
    pipes = {(ch, lay): bench.make_pipeline(wl, B, 0, None, frame_dtype="uint8", frame_channels=ch, frame_layout=lay)
             for ch in (1, 3) for lay in ("packed", "strided")}
    maps = pipes[(1, "packed")]._alloc_maps()
    for p in pipes.values():
        p._adopt_maps(dict(maps))
    views = make_views(B, h, w, gray, colour)
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls, "layouts": {},
                    "library": os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so")}
    for lay, (view, ch) in views.items():
        assert not view.is_contiguous()
        packed = view.contiguous()
        second = torch.empty_like(packed)
        pp, ps = pipes[(ch, "packed")], pipes[(ch, "strided")]

        def pack_step():
            second.copy_(view)
            pp.step(second)

        variants = {"packed": lambda: pp.step(packed), "pack_step": pack_step, "strided": lambda: ps.step(view)}
        digests = {}
        for k in ("pack_step", "strided"):
            for m in maps.values():
                m.fill_(-7.0)
            variants[k]()
            torch.cuda.synchronize()
            digests[k] = [int(m.view(torch.int32).to(torch.int64).sum().item()) for m in maps.values()]
        assert digests["pack_step"] == digests["strided"], (lay, digests)
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
        lines = lines_per_frame(view, ch, h, w) * 128
        model = {"packed": model_bytes(pp, h * w * ch), "pack_step": model_bytes(pp, h * w * ch, before=lines + h * w * ch),
                 "strided": model_bytes(ps, lines)}
        result[name]["layouts"][lay] = {
            "channels": ch, "view": list(_runtime.frame_view_of(view, ch)[1:]),
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
            "strided_over_pack_step": round(med["strided"] / med["pack_step"], 4),
            "strided_over_packed": round(med["strided"] / med["packed"], 4),
            "claim_strided_below_pack_step": bool(med["strided"] < med["pack_step"]),
            "model_bytes_per_frame": model,
            "model_byte_ratio": {"strided_over_pack_step": round(model["strided"]["step"] / model["pack_step"]["step"], 4),
                                 "strided_over_packed": round(model["strided"]["step"] / model["packed"]["step"], 4)},
            "second_buffer_bytes": int(second.numel()), "pack_step_and_strided_outputs_bit_identical": True}
        del packed, second, variants
    for p in pipes.values():
        p.close()
    del pipes, maps, views, colour, gray
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
