#!/usr/bin/env python3
"""What a COLOUR uint8 source costs the gray step (LineEndPipeline(mode="gray", frame_dtype="uint8", frame_channels=3)), in ONE
process AT THE SAME ADDRESSES (placement=None; the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md):
the three pipelines of a workload ADOPT THE SAME pyramid, CS and end buffers; timing windows alternate between the variants.
The colour frames are bench.py's seeded frames with three channels (uint8 values), resident as [B, H, W, 3] uint8.

    python scripts/time_gray_rgb8.py [config2 config5 ...]   [CALLS=5] [STEPS=20] [HOST_CALLS=6]

Per workload, min / median / max ms per step of
    gray_uint8     (a) the uint8 single-channel step on a PRECOMPUTED uint8 gray frame: the floor (nothing in the library produces
                       such a frame from colour; it is made outside the timed region)
    cast_value     (b) what a colour uint8 source costs without frame_channels=3: the widening cast of the resident colour frames
                       (silent_cast_interleave_dev, 3 -> 12 B/px), the value kernel (silent_value_from_color_dev, 12 -> 4 B/px) and
                       the float32-frame step
    colour_uint8   (c) the colour step on the resident colour frames (3 B/px read, value formed at the load)
and the byte ratios of DESIGN.md section 4.2's per-pixel model they are held against (level 0 of (c): 3 + 4 + 4 (1 + K) B/px; (b)
moves 31 B per frame pixel in two launches before its step starts, and that step then reads 4 B/px where (c) reads 3).  (b) and
(c) write the same buffers and must leave the same bits.
Separately: step_host frames / s from PINNED colour host frames through (c) and through (b)'s path (a two-slot ring like
step_host's: H2D on a copy stream, then cast + value + float32 step), and the device bytes each ingest holds.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from pysilent_amd import _lib, _runtime
from pysilent_amd import distributed as D

names = sys.argv[1:] or ["config2", "config5"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
host_calls = int(os.environ.get("HOST_CALLS", "6"))
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = _lib.load()


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def model_bytes(pipe, frame_bytes, extra=0):
    """DESIGN 4.2's bytes per frame: gray_stream_kernel (frame read, pyramid of every level, CS + end of level 0) and
    gray_line_end_kernel (pyramid read, CS + end of the other levels); extra: bytes per frame pixel moved before the step."""
    K = pipe.n_orient
    px0 = pipe.extents[0][0] * pipe.extents[0][1]
    rest = pipe.frame_px - px0
    stream = px0 * (frame_bytes + 4 + 4 * (1 + K)) + rest * 4
    line_end = rest * (4 + 4 * (1 + K))
    return {"gray_stream_kernel": stream, "gray_line_end_kernel": line_end, "before_the_step": px0 * extra,
            "step": stream + line_end + px0 * extra}


class CastValuePath(object):
    """(b): colour uint8 frames -> float32 colour (cast kernel) -> float32 value frame (value kernel) -> the float32-frame step."""

    def __init__(self, pipe, B, h, w):
        self.pipe, self.n_px, self.B = pipe, B * h * w, B
        self.f32x3 = torch.empty((B, h, w, 3), dtype=torch.float32, device=dev)
        self.value = torch.empty((B, h, w, 1), dtype=torch.float32, device=dev)
        self.level = (_lib.Extent * 1)(_lib.Extent(h, w))
        self.ctx = _runtime.get_context(0)

    def __call__(self, rgb8):
        _runtime.cast_interleave(rgb8, self.f32x3, 3, 0, 3, 3, 0, self.n_px)
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.ctx.check(lib.silent_value_from_color_dev(self.ctx.handle, C.c_void_p(self.f32x3.data_ptr()), self.level, 1, self.B, 3,
                                                       C.c_void_p(self.value.data_ptr()), s))
        self.pipe.step(self.value)

    def device_bytes(self):
        return int(self.f32x3.numel() * 4 + self.value.numel() * 4)


def host_rate_colour(pipe, src, B):
    """step_host frames / s of the colour pipeline: two batches to fill the ring, then ``host_calls`` batches on the host clock."""
    for _ in range(2):
        pipe.step_host(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(host_calls):
        pipe.step_host(src)
    pipe.wait()
    torch.cuda.synchronize()
    return B * host_calls / (time.perf_counter() - t0)


def host_rate_cast_value(path, src, B):
    """The same source through (b)'s path: a ring of two uint8 device buffers filled on a copy stream, cast + value + step behind."""
    copy = torch.cuda.Stream(dev)
    cur = torch.cuda.current_stream(dev)
    raw = [torch.empty(tuple(src.shape), dtype=torch.uint8, device=dev) for _ in range(2)]
    done = [torch.cuda.Event() for _ in range(2)]
    free = [None, None]

    def one(i):
        k = i & 1
        if free[k] is not None:
            copy.wait_event(free[k])
        with torch.cuda.stream(copy):
            raw[k].copy_(src, non_blocking=True)
        done[k].record(copy)
        cur.wait_event(done[k])
        path(raw[k])
        free[k] = torch.cuda.Event()
        free[k].record(cur)

    for i in range(2):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(host_calls):
        one(i)
    path.pipe.wait()
    torch.cuda.synchronize()
    rate = B * host_calls / (time.perf_counter() - t0)
    return rate, int(sum(t.numel() for t in raw))


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    assert wl["mode"] == "gray", name
    B = wl["frames"]
    h, w = wl["hw"]
    pipes = {"float32": bench.make_pipeline(wl, B, 0, None), "uint8": bench.make_pipeline(wl, B, 0, None, frame_dtype="uint8"),
             "colour": bench.make_pipeline(wl, B, 0, None, frame_dtype="uint8", frame_channels=3)}
    host = np.stack([D.synthetic_frame(gi, h, w, 3) for gi in D.shard_frame_indices(B, 0, 1)])
    rgb8_host = host.astype(np.uint8)
    assert np.array_equal(rgb8_host.astype(host.dtype), host), "the seeded frames are uint8 values"
    del host
    rgb8 = torch.from_numpy(rgb8_host).to(dev)
    path = CastValuePath(pipes["float32"], B, h, w)
    # (a)'s frame: a uint8 gray frame made outside the timed region (the value rounded to a byte)
    _runtime.cast_interleave(rgb8, path.f32x3, 3, 0, 3, 3, 0, B * h * w)
    gray8 = _runtime.value_from_color(path.f32x3).round().to(torch.uint8).contiguous()
    maps = pipes["float32"]._alloc_maps()
    for p in pipes.values():
        p._adopt_maps(dict(maps))

    variants = {"gray_uint8": lambda: pipes["uint8"].step(gray8), "cast_value": lambda: path(rgb8),
                "colour_uint8": lambda: pipes["colour"].step(rgb8)}
    # (b) and (c) write the same buffers: their results must be the same bits
    digests = {}
    for k in ("cast_value", "colour_uint8"):
        for m in maps.values():
            m.fill_(-7.0)
        variants[k]()
        torch.cuda.synchronize()
        digests[k] = [int(m.view(torch.int32).to(torch.int64).sum().item()) for m in maps.values()]
    assert digests["cast_value"] == digests["colour_uint8"], digests
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
    model = {"gray_uint8": model_bytes(pipes["uint8"], 1), "cast_value": model_bytes(pipes["float32"], 4, extra=3 + 12 + 12 + 4),
             "colour_uint8": model_bytes(pipes["colour"], 3)}
    # ingest: pinned colour host frames through (c)'s step_host and through (b)'s path
    pinned = torch.from_numpy(rgb8_host).pin_memory()
    rate_c = host_rate_colour(pipes["colour"], pinned, B)
    slots = pipes["colour"]._ingest[torch.uint8]["slots"]
    ring_c = int(sum(t.numel() * t.element_size() for s in slots for t in (s["raw"], s["f32"]) if t is not None))
    rate_b, raw_b = host_rate_cast_value(path, pinned, B)
    result[name] = {"frames": B, "steps_per_call": steps, "calls": calls,
                    "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
                    "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
                    "colour_over_cast_value": round(med["colour_uint8"] / med["cast_value"], 4),
                    "colour_over_gray_uint8": round(med["colour_uint8"] / med["gray_uint8"], 4),
                    "model_bytes_per_frame": model,
                    "model_byte_ratio": {"colour_over_cast_value": round(model["colour_uint8"]["step"] / model["cast_value"]["step"], 4),
                                         "colour_over_gray_uint8": round(model["colour_uint8"]["step"] / model["gray_uint8"]["step"], 4)},
                    "step_host_pinned_colour_frames_per_s": {"cast_value": round(rate_b, 1), "colour_uint8": round(rate_c, 1)},
                    "ingest_device_bytes": {"cast_value": raw_b + path.device_bytes(), "colour_uint8": ring_c},
                    "host_calls": host_calls, "resident_frame_bytes": int(rgb8.numel()),
                    "cast_value_and_colour_outputs_bit_identical": True,
                    "library": os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so"),
                    "streamable": {k: p.plan.streamable for k, p in pipes.items()}}
    for p in pipes.values():
        p.close()
    del pipes, maps, rgb8, gray8, path, variants, pinned, rgb8_host
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
