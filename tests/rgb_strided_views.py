"""The views of the strided uint8 colour tests (tests/test_rgb_strided.py on the GPU, tests/test_rgb_strided_host.py for the mistake
model; test infrastructure, like tests/rgb_uint8_frames.py, whose batches these views carry).

A view kind is a LAYOUT: the byte offset of channel 0 of pixel (0, 0) of frame 0 inside a flat uint8 PARENT buffer, and the three byte
strides (frame, row, pixel).  place() writes a packed batch [B, H, W, 3] through the layout into a parent filled with one byte value
-- 0x00 or 0xFF: a byte that is not the view's but changes a result shows under one of the two fills -- and as_numpy / as_torch give
the [B, H, W, 3] view of a parent (host ndarray / GPU tensor), nothing copied."""
import numpy as np

KINDS = ("bgra", "bgra at byte 1", "odd-pitch bgr", "region at (7, 5)", "every second pixel", "frames with a gap", "packed")
FILLS = (0x00, 0xFF)


def layout(kind, B, H, W):
    """(parent size in bytes, offset, frame stride, row stride, pixel stride) of ``kind`` for a batch [B, H, W, 3]."""
    if kind == "bgra":                     # 3 of 4 bytes, the parent 4-byte aligned
        return B * H * W * 4, 0, H * W * 4, W * 4, 4
    if kind == "bgra at byte 1":           # the same at byte offset 1 of a larger allocation
        return B * H * W * 4 + 8, 1, H * W * 4, W * 4, 4
    if kind == "odd-pitch bgr":
        row = 3 * W + 5
        return B * H * row, 0, H * row, row, 3
    if kind == "region at (7, 5)":         # of [B, H + 20, W + 13, 3] parents: odd offset, odd pitch
        row = 3 * (W + 13)
        return B * (H + 20) * row, 7 * row + 5 * 3, (H + 20) * row, row, 3
    if kind == "every second pixel":       # of a [B, H, 2 W, 3] parent
        return B * H * W * 6, 0, H * W * 6, W * 6, 6
    if kind == "frames with a gap":        # separate slices of one buffer
        frame = H * W * 3 + 1001
        return B * frame + 3, 3, frame, W * 3, 3
    if kind == "packed":
        return B * H * W * 3, 0, H * W * 3, W * 3, 3
    raise KeyError(kind)


def span(kind, B, H, W):
    _, _, sf, sr, sp = layout(kind, B, H, W)
    return (B - 1) * sf + (H - 1) * sr + (W - 1) * sp + 3


def as_numpy(parent, kind, B, H, W):
    _, off, sf, sr, sp = layout(kind, B, H, W)
    return np.lib.stride_tricks.as_strided(parent[off:], (B, H, W, 3), (sf, sr, sp, 1), writeable=parent.flags.writeable)


def as_torch(parent, kind, B, H, W):
    import torch
    _, off, sf, sr, sp = layout(kind, B, H, W)
    return torch.as_strided(parent, (B, H, W, 3), (sf, sr, sp, 1), off)


def place(kind, frames, fill):
    """The flat parent of ``kind`` filled with ``fill`` and carrying ``frames`` [B, H, W, 3] uint8."""
    B, H, W, _ = frames.shape
    parent = np.full(layout(kind, B, H, W)[0], fill, np.uint8)
    as_numpy(parent, kind, B, H, W)[...] = frames
    return parent


# ----------------------------------------------------------------------------- the mistakes a strided byte loader can make
# Each takes (parent, kind, B, H, W) and returns the float32 frames [B, H, W, 3] a kernel with that mistake would see; an address past
# the parent wraps into it (what lies there is somebody else's memory).

def _gather(parent, off, sf, sr, sp, B, H, W, ch0=0):
    f, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return np.take(parent, (off + f * sf + y * sr + x * sp + c + ch0) % parent.size).astype(np.float32)


def truth(parent, kind, B, H, W):
    _, off, sf, sr, sp = layout(kind, B, H, W)
    return _gather(parent, off, sf, sr, sp, B, H, W)


def pixel_stride_3(parent, kind, B, H, W):
    _, off, sf, sr, _ = layout(kind, B, H, W)
    return _gather(parent, off, sf, sr, 3, B, H, W)


def row_stride_from_pixels(parent, kind, B, H, W):
    _, off, sf, _, sp = layout(kind, B, H, W)
    return _gather(parent, off, sf, W * sp, sp, B, H, W)


def frame_stride_packed(parent, kind, B, H, W):
    _, off, _, sr, sp = layout(kind, B, H, W)
    return _gather(parent, off, H * sr, sr, sp, B, H, W)


def channel_offset_1(parent, kind, B, H, W):
    _, off, sf, sr, sp = layout(kind, B, H, W)
    return _gather(parent, off, sf, sr, sp, B, H, W, ch0=1)


def base_aligned_down(parent, kind, B, H, W):
    _, off, sf, sr, sp = layout(kind, B, H, W)
    return _gather(parent, off & ~3, sf, sr, sp, B, H, W)


MISTAKES = {"pixel stride taken as 3": pixel_stride_3, "row stride taken as W * pixel_stride": row_stride_from_pixels,
            "frame stride taken as packed": frame_stride_packed, "channel offset +1": channel_offset_1,
            "base aligned down to a dword": base_aligned_down}
# the kinds on which a mistake is a mistake at all (on the others it changes no address)
VISIBLE_ON = {"pixel stride taken as 3": ("bgra", "bgra at byte 1", "every second pixel"),
              "row stride taken as W * pixel_stride": ("odd-pitch bgr", "region at (7, 5)"),
              "frame stride taken as packed": ("region at (7, 5)", "frames with a gap"),
              "channel offset +1": tuple(k for k in KINDS if k != "packed"),
              "base aligned down to a dword": ("bgra at byte 1", "region at (7, 5)", "frames with a gap")}
