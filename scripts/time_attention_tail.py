#!/usr/bin/env python3
"""What the attention tail (LineEndPipeline(mode="rgb", attention=True): centroids at two scales + the boosting state per frame slot,
silent_attention_tail_dev) costs on top of the RGB step, against the per-op sequence it replaces, in ONE process AT THE SAME ADDRESSES
(placement=None; the pipelines of a workload ADOPT THE SAME pyramid and map buffers, the fused tail and the per-op sequence write the same
four result buffers); timing windows alternate between the legs, device events around each window.  The method of scripts/time_rgb_nv12.py.

    python scripts/time_attention_tail.py [reference_layout config3 ...]   [CALLS=5] [STEPS=20]

Per workload, min / median / max ms of
    step            (a) the step with attention=False (value map kept: the tail reads it)
    step_per_op     (b) (a) + the per-op sequence (4 affine launches on maps, 2 centroid calls, a resize, a boosting call ...: ten *_dev calls)
                        into PREALLOCATED buffers on the same stream: what the capability costs without the fused tail
    step_attention  (c) the step with attention=True
    tail, per_op    the fused tail and the per-op sequence alone, on the value map the last step left
beside the byte model of the tail (attention_bytes_per_frame) and its time at the measured copy rate.  Prints one JSON line."""
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

names = sys.argv[1:] or ["reference_layout", "config3"]
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


def copy_rate():
    """Bytes moved per ms (read + write) by a device-to-device copy of 1 GiB: the rate the byte model is priced at."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    src.fill_(1.0)
    for _ in range(3):
        dst.copy_(src)
    ms = min(timed(lambda: dst.copy_(src), 5) for _ in range(3))
    return 2.0 * src.numel() * 4 / ms


class PerOp(object):
    """The per-op sequence of include/silent_hip.h (silent_attention_tail's definition) through the *_dev entry points, every
    intermediate and result preallocated; the four results go to ``pipe``'s own result buffers."""

    def __init__(self, pipe):
        self.p, self.ctx, self.lib = pipe, pipe.ctx, _lib.load()
        n, f32 = pipe.batch, dict(dtype=torch.float32, device=dev)
        ext = lambda e: (_lib.Extent * len(e))(*[_lib.Extent(h, w) for h, w in e])
        self.levels, self.half, self.cells, self.cells2 = (ext(e) for e in (pipe.extents, pipe.attention_half, pipe.attention_cells, pipe.attention_cells2))
        px, px2 = n * pipe.frame_px, n * sum(h * w for h, w in pipe.attention_half)
        nc, nc2, c = n * pipe.cells_per_frame, n * sum(h * w for h, w in pipe.attention_cells2), pipe.attention_channels
        self.g, self.dist, self.tot, self.imp = (torch.empty(k, **f32) for k in (px, px, nc, nc))
        self.im2, self.im2n, self.dist2, self.tot2 = (torch.empty(k, **f32) for k in (px2, px2, px2, nc2))
        self.fired = torch.empty(nc * c, **f32)
        self.energy = torch.full((nc,), 8.0, **f32)
        self.device_bytes = 4 * (3 * px + 3 * px2 + 2 * nc + nc2 + nc * c)
        A = _lib.AffineParams
        inf = float("inf")
        self.by255, self.to_imp = A(1.0, 255.0, 0.0, -inf, inf, 0.0), A(255 / 4.0, 1.0, 0.0, 1.0, 256.0, -1.0)
        self.inv, self.x255 = A(-255.0, 1.0, 255.0, -inf, inf, 0.0), A(255.0, 1.0, 0.0, -inf, inf, 0.0)

    def __call__(self):
        p, lib, h = self.p, self.lib, self.p.ctx.handle
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        q = lambda t: C.c_void_p(t.data_ptr())
        n, L, ap = p.batch, p.n_levels, p._attention_params
        ck = self.ctx.check
        ck(lib.silent_affine_clip_dev(h, q(p.value), self.g.numel(), C.byref(self.by255), q(self.g), s))
        ck(lib.silent_centroids_dev(h, q(self.g), self.levels, L, n, ap.region_h, ap.region_w, q(self.dist), q(self.tot), s))
        ck(lib.silent_affine_clip_dev(h, q(self.tot), self.tot.numel(), C.byref(self.to_imp), q(self.imp), s))
        ck(lib.silent_resize_nearest_dev(h, q(p.value), self.levels, L, n, 1, self.half, q(self.im2), s))
        ck(lib.silent_affine_clip_dev(h, q(self.im2), self.im2.numel(), C.byref(self.by255), q(self.im2n), s))
        ck(lib.silent_centroids_dev(h, q(self.im2n), self.half, L, n, ap.region_h, ap.region_w, q(self.dist2), q(self.tot2), s))
        ck(lib.silent_boosting_step_dev(h, q(self.imp), self.cells, L, n, C.byref(ap.boosting), q(self.energy), q(self.fired), q(p.update), s))
        ck(lib.silent_affine_clip_dev(h, q(self.dist), self.dist.numel(), C.byref(self.inv), q(p.centroids), s))
        ck(lib.silent_affine_clip_dev(h, q(self.dist2), self.dist2.numel(), C.byref(self.inv), q(p.centroids2), s))
        ck(lib.silent_affine_clip_dev(h, q(self.fired), self.fired.numel(), C.byref(self.x255), q(p.fired), s))


result = {"copy_rate_bytes_per_ms": copy_rate()}
for name in names:
    wl = bench.WORKLOADS[name]
    B = wl["frames"]
    kw = dict(value_map=True, peak_value_map=False)
    pipes = {"off": bench.make_pipeline(wl, B, 0, None, **kw), "on": bench.make_pipeline(wl, B, 0, None, attention=True, **kw)}
    frames = bench.make_frames(torch, D, wl, B, 0, 1, dev)
    off, on = pipes["off"], pipes["on"]
    maps = {k: v for k, v in on._alloc_maps().items() if v is not None}
    for p in pipes.values():
        p._adopt_maps(dict(maps))
    per_op = PerOp(on)
    outs = (on.centroids, on.centroids2, on.fired, on.update)

    def step_per_op():
        off.step(frames)
        per_op()

    variants = {"step": lambda: off.step(frames), "step_per_op": step_per_op, "step_attention": lambda: on.step(frames),
                "tail": lambda: on.run_attention(), "per_op": per_op}
    # (b) and (c) write the same result buffers from the same state: the same bits, results and advanced state
    digests = {}
    for k in ("step_per_op", "step_attention"):
        for t in outs:
            t.fill_(-7.0)
        on.reset_state()
        per_op.energy.fill_(8.0)
        for _ in range(2):
            variants[k]()
        torch.cuda.synchronize()
        state = on.energy.reshape(-1) if k == "step_attention" else per_op.energy
        digests[k] = [int(t.view(torch.int32).to(torch.int64).sum().item()) for t in outs + (state,)]
    assert digests["step_per_op"] == digests["step_attention"], digests
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
    tail_bytes = on.attention_bytes_per_frame() * B
    model_ms = tail_bytes / result["copy_rate_bytes_per_ms"]
    result[name] = {
        "frames": B, "steps_per_call": steps, "calls": calls, "levels": [list(e) for e in on.extents], "half_levels": [list(e) for e in on.attention_half],
        "cells_per_frame": on.cells_per_frame, "launch_summary": on.launch_summary(),
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
        "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
        "windows_ms": {k: [round(float(x), 4) for x in v] for k, v in ms.items()},
        "every_attention_window_below_every_per_op_window": bool(np.max(ms["step_attention"]) < np.min(ms["step_per_op"])),
        "attention_over_per_op": round(med["step_attention"] / med["step_per_op"], 4),
        "tail_cost_ms": {"fused_c_minus_a": round(med["step_attention"] - med["step"], 4), "per_op_b_minus_a": round(med["step_per_op"] - med["step"], 4)},
        "frames_per_s": {"step": round(B / med["step"] * 1e3), "step_per_op": round(B / med["step_per_op"] * 1e3),
                         "step_attention": round(B / med["step_attention"] * 1e3)},
        "tail_model": {"bytes_per_step": int(tail_bytes), "ms_at_copy_rate": round(model_ms, 4),
                       "fused_cost_over_model": round((med["step_attention"] - med["step"]) / model_ms, 3),
                       "tail_alone_over_model": round(med["tail"] / model_ms, 3)},
        "per_op_intermediate_device_bytes": per_op.device_bytes,
        "tail_workspace_bytes": B * (16 * on.cells_per_frame + 8 * sum(h * w for h, w in on.attention_cells2)),
        "outputs_bit_identical": True}
    for p in pipes.values():
        p.close()
    del pipes, off, on, maps, frames, per_op, outs, variants
    torch.cuda.empty_cache()
print(json.dumps(result), flush=True)
