"""The frames of the packed uint8 colour tests (tests/test_rgb_uint8.py on the GPU, tests/test_rgb_uint8_host.py for the mistake model;
test infrastructure, like tests/plan_geometry.py).

A batch [B, H, W, 3] uint8: noise from rng.integers(0, 256), the LAST frame a ramp (3 x + c + 7 y) % 256 -- neighbouring bytes differ
by one, so an address that is off by a byte, a row start rounded down to a dword, or a swapped channel changes every value a
little and none by a multiple of 256 --, and in every frame the bytes 0, 255, 128 at the first and last pixel of rows 0 and H - 1
(the batch's first and last bytes are known, and 128 / 255 are negative as signed bytes)."""
import numpy as np

CORNER = (0, 255, 128)


def batch(B, H, W, seed=0):
    rng = np.random.default_rng(7300 + seed)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    frames[B - 1] = ((3 * x + c + 7 * y) % 256).astype(np.uint8)
    for yy in (0, H - 1):
        for xx in (0, W - 1):
            frames[:, yy, xx] = CORNER
    return frames


# ----------------------------------------------------------------------------- the mistakes a byte loader can make
# Each takes the batch and returns the float32 frames a kernel with that mistake would see (same shape).  The flat byte buffer is the
# batch followed by 3 bytes of 0xA5 -- what lies behind it in a larger allocation.

def widened(frames):
    return frames.astype(np.float32)


def signed_bytes(frames):
    return frames.view(np.int8).astype(np.float32)


def channels_reversed(frames):
    return frames[..., ::-1].astype(np.float32)


def _flat(frames):
    return np.concatenate([frames.reshape(-1), np.full(3, 0xA5, np.uint8)])


def float_sized_frame_stride(frames):
    """Frame f >= 1 addressed f * H * W * 3 * 4 bytes behind frame 0 (the stride of the float32 batch), wrapped inside the batch."""
    B, n = frames.shape[0], frames[0].size
    flat = frames.reshape(-1)
    out = np.stack([np.take(flat, (4 * f * n + np.arange(n)) % flat.size) for f in range(B)])
    return out.reshape(frames.shape).astype(np.float32)


def row_residue_dropped(frames):
    """Every row start rounded down to a multiple of 4 bytes (an aligned-down dword load): rows whose start has 3 W y mod 4 != 0
    are read 1 - 3 bytes early."""
    B, H, W, _ = frames.shape
    flat = _flat(frames)
    out = np.empty(frames.shape, np.uint8)
    for f in range(B):
        for y in range(H):
            start = ((f * H + y) * W * 3) & ~3
            out[f, y] = flat[start:start + 3 * W].reshape(W, 3)
    return out.astype(np.float32)


def one_byte_offset(frames):
    flat = _flat(frames)
    return flat[1:1 + frames.size].reshape(frames.shape).astype(np.float32)


MISTAKES = {"signed bytes": signed_bytes, "channel order reversed": channels_reversed,
            "float-sized frame stride": float_sized_frame_stride, "row-start residue dropped": row_residue_dropped,
            "one byte of offset": one_byte_offset}
