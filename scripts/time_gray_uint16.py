#!/usr/bin/env python3
"""float32 frames against uint16 frames for the gray step (LineEndPipeline(mode="gray", frame_dtype=...)), in ONE process AT THE
SAME ADDRESSES (placement=None; the placement of the maps moves a step by up to 25 %, profiles/r06/placement.md): every pipeline
of a workload ADOPTS THE SAME pyramid, CS and end buffers; the frames are bench.py's seeded frames times 257 (0 .. 65535, exact in
both types; clip_hi = 65535 for every pipeline); timing windows alternate between the variants.

    python scripts/time_gray_uint16.py [config2 config5 ...]   [CALLS=5] [STEPS=20] [HOST_CALLS=6]

Per workload, min / median / max ms per step of
    float32        (a) the float32-frame step on resident float32 frames
    cast_float32   (b) the widening cast of the resident uint16 frames (silent_cast_interleave_dev) + the float32-frame step: what a
                       resident uint16 source costs without frame_dtype="uint16" -- kernels that exist without this frame kind
    uint16         (c) the uint16-frame step on the resident uint16 frames
CRITERION: every window of (c) lies below every window of (b).  c / a is reported beside the byte ratio of DESIGN.md section 4.2's
per-pixel model (level 0: 2 instead of 4 bytes read + 4 pyramid + CS + K end; other levels unchanged), without a threshold.
One pitched layout, surface[:, :H, :W] of [B, H * 3 / 2, pitch] uint16 surfaces (P010 luma; pitch = W rounded up to a power of two):
    packed         the packed uint16 step on a precomputed packed copy
    pack_step      one launch that packs the view into a preallocated second buffer, then the packed step
    strided        the strided step on the view (frame_layout="strided")
Separately: step_host frames / s from pinned uint16 host frames on the uint16 pipeline and on the float32 pipeline (upload, widening
cast into a float32 slot buffer, step), and the device bytes of the ingest ring each of them holds.  Each GPU step of a job that runs
this script gets its own time limit from the caller.  Prints one JSON line."""
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

names = sys.argv[1:] or ["config2", "config5"]
calls, steps = int(os.environ.get("CALLS", "5")), int(os.environ.get("STEPS", "20"))
host_calls = int(os.environ.get("HOST_CALLS", "6"))
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
FULL = 65535.0


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def model_bytes(pipe, frame_bytes):
    """DESIGN 4.2's bytes per frame: gray_stream_kernel (frame read, pyramid of every level, CS + end of level 0) and
    gray_line_end_kernel (pyramid read, CS + end of the other levels)."""
    K = pipe.n_orient
    px0 = pipe.extents[0][0] * pipe.extents[0][1]
    rest = pipe.frame_px - px0
    stream = px0 * (frame_bytes + 4 + 4 * (1 + K)) + rest * 4
    line_end = rest * (4 + 4 * (1 + K))
    return {"gray_stream_kernel": stream, "gray_line_end_kernel": line_end, "step": stream + line_end}


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
    slots = pipe._ingest[torch.uint16]["slots"]
    return int(sum(t.numel() * t.element_size() for s in slots for t in (s["raw"], s["f32"]) if t is not None))


def windows(variants, maps, same):
    """The variants in `same` must leave the same bits; then `calls` alternating windows of `steps` steps each."""
    digests = {}
    for k in same:
        for m in maps.values():
            m.fill_(-7.0)
        variants[k]()
        torch.cuda.synchronize()
        digests[k] = [int(m.view(torch.int32).to(torch.int64).sum().item()) for m in maps.values()]
    assert all(d == digests[same[0]] for d in digests.values()), digests
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
    return ms


def stats(ms):
    return {"median_ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
            "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()}}


result = {}
for name in names:
    wl = bench.WORKLOADS[name]
    assert wl["mode"] == "gray", name
    B = wl["frames"]
    h, w = wl["hw"]
    host16 = (bench.make_frames(torch, D, wl, B, 0, 1, dev).cpu().numpy().astype(np.uint16) * np.uint16(257))
    assert host16.dtype == np.uint16 and host16.max() > 32767
    u16 = torch.from_numpy(host16).to(dev)
    frames = torch.from_numpy(host16.astype(np.float32)).to(dev)
    pipes = {(fd, lay): bench.make_pipeline(wl, B, 0, None, frame_dtype=fd, clip_hi=FULL, **({"frame_layout": lay} if lay == "strided" else {}))
             for fd, lay in (("float32", "packed"), ("uint16", "packed"), ("uint16", "strided"))}
    pf, pu, ps = pipes[("float32", "packed")], pipes[("uint16", "packed")], pipes[("uint16", "strided")]
    cast_buf = torch.empty_like(frames)
    maps = pf._alloc_maps()
    for p in pipes.values():
        p._adopt_maps(dict(maps))
    n_px = frames.numel()

    def cast_then_step():
        _runtime.cast_interleave(u16, cast_buf, 1, 0, 1, 1, 0, n_px)
        pf.step(cast_buf)

    ms = windows({"float32": lambda: pf.step(frames), "cast_float32": cast_then_step, "uint16": lambda: pu.step(u16)}, maps,
                 ("float32", "cast_float32", "uint16"))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    model = {"float32": model_bytes(pf, 4), "uint16": model_bytes(pu, 2)}

    # one pitched layout: P010 luma
    pitch = 1 << (w - 1).bit_length()
    surface_host = np.full((B, h * 3 // 2, pitch), 0x8000, np.uint16)
    surface_host[:, :h, :w] = host16[..., 0]
    surface = torch.from_numpy(surface_host).to(dev)
    del surface_host
    view = surface[:, :h, :w]
    assert not view.is_contiguous()
    second = torch.empty_like(u16)

    def pack_step():
        second.view(torch.int16)[..., 0].copy_(view.view(torch.int16))      # (the same bytes as a uint16 copy)
        pu.step(second)

    ms_p = windows({"packed": lambda: pu.step(u16), "pack_step": pack_step, "strided": lambda: ps.step(view)}, maps,
                   ("packed", "pack_step", "strided"))
    med_p = {k: float(np.median(v)) for k, v in ms_p.items()}

    # ingest: pinned uint16 host frames through step_host of the uint16 pipeline and of the float32 pipeline
    host_pinned = torch.from_numpy(host16).pin_memory()
    ingest = {}
    for k, p in (("uint16", pu), ("float32", pf)):
        ingest[k] = {"pinned_frames_per_s": round(host_rate(p, host_pinned, B), 1), "ring_device_bytes": ring_bytes(p)}
    result[name] = dict(stats(ms), frames=B, steps_per_call=steps, calls=calls,
                        criterion_every_uint16_window_below_every_cast_float32_window=bool(max(ms["uint16"]) < min(ms["cast_float32"])),
                        uint16_over_float32=round(med["uint16"] / med["float32"], 4),
                        uint16_over_cast_float32=round(med["uint16"] / med["cast_float32"], 4),
                        model_bytes_per_frame=model,
                        model_byte_ratio={k: round(model["uint16"][k] / model["float32"][k], 4) for k in model["float32"]},
                        pitched=dict(stats(ms_p), view=list(_runtime.frame_view_of(view, 1)[1:]),
                                     every_strided_window_below_every_pack_step_window=bool(max(ms_p["strided"]) < min(ms_p["pack_step"])),
                                     strided_over_pack_step=round(med_p["strided"] / med_p["pack_step"], 4),
                                     strided_over_packed=round(med_p["strided"] / med_p["packed"], 4), second_buffer_bytes=int(second.numel() * 2)),
                        step_host_uint16_frames=ingest, host_calls=host_calls,
                        resident_frame_bytes={"float32": int(frames.numel() * 4), "uint16": int(u16.numel() * 2)},
                        outputs_bit_identical=True,
                        library=os.path.basename(os.environ.get("SILENT_LIB_PATH") or "libsilent_hip.so"),
                        streamable={"%s %s" % k: p.plan.streamable for k, p in pipes.items()})
    for p in pipes.values():
        p.close()
    del pipes, pf, pu, ps, maps, frames, u16, cast_buf, surface, view, second, host_pinned, host16
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
