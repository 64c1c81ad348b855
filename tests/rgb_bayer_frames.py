"""The data of the raw Bayer mosaic tests (tests/test_rgb_bayer.py on the GPU, tests/test_rgb_bayer_host.py without one; test
infrastructure, like tests/rgb_yuv_frames.py).

A LAYOUT says where the bytes m(f, y, x) of a batch of mosaics lie: the size of one flat PARENT, the byte offset of pixel (0, 0, 0)
inside it and the (frame, row, pixel) byte strides.  place() puts the mosaic into a parent filled with one byte value (0x00, then
0xFF: a byte that is no pixel's but changes a result shows under one of the two fills); view() / torch_view() return the [n, H, W]
view.  The INDEPENDENT ORACLE is truth(): the words of include/silent_hip.h restated with np.pad(mode="reflect") and slicing -- it
knows nothing of the kernels.  checks() are the three statements the restatement must pass before anything is compared with it."""
import numpy as np

FILLS = (0x00, 0xFF)
PATTERNS = ("rggb", "grbg", "gbrg", "bggr")           # pattern 0 .. 3 of silent_bayer_frames
ORDERS = ("bgr", "rgb")
RED = {"rggb": (0, 0), "grbg": (0, 1), "gbrg": (1, 0), "bggr": (1, 1)}    # red at (y & 1, x & 1); blue on the other diagonal site


def truth(m, pattern, order="bgr"):
    """[n, H, W] uint8 mosaics -> [n, H, W, 3] float32: bilinear demosaicing, indices outside the frame reflected without repeating
    the edge; every sum an integer, converted once and multiplied once by 0.25 or 0.5."""
    m = np.asarray(m)
    assert m.dtype == np.uint8 and m.ndim == 3 and m.shape[1] >= 2 and m.shape[2] >= 2
    n, H, W = m.shape
    p = np.pad(m.astype(np.int64), ((0, 0), (1, 1), (1, 1)), mode="reflect")
    c = p[:, 1:-1, 1:-1]
    up, down, left, right = p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]
    diag = p[:, :-2, :-2] + p[:, :-2, 2:] + p[:, 2:, :-2] + p[:, 2:, 2:]
    f = np.float32
    own = c.astype(f)
    cross = (up + down + left + right).astype(f) * f(0.25)
    diagonal = diag.astype(f) * f(0.25)
    horizontal = (left + right).astype(f) * f(0.5)
    vertical = (up + down).astype(f) * f(0.5)
    ry, rx = RED[pattern]
    yy, xx = np.arange(H)[:, None] & 1, np.arange(W)[None, :] & 1
    at_red = np.broadcast_to((yy == ry) & (xx == rx), (H, W))
    at_blue = np.broadcast_to((yy != ry) & (xx != rx), (H, W))
    red_row = np.broadcast_to((yy == ry) & (xx != rx), (H, W))        # a green site whose row holds the red samples
    g = np.where(at_red | at_blue, cross, own)
    r = np.where(at_red, own, np.where(at_blue, diagonal, np.where(red_row, horizontal, vertical)))
    b = np.where(at_blue, own, np.where(at_red, diagonal, np.where(red_row, vertical, horizontal)))
    assert order in ORDERS
    return np.stack((b, g, r) if order == "bgr" else (r, g, b), axis=-1).astype(np.float32)


def constant_mosaic(H, W, pattern, rgb):
    """The mosaic a sensor of this pattern records of a field of one colour (r, g, b)."""
    ry, rx = RED[pattern]
    yy, xx = np.arange(H)[:, None] & 1, np.arange(W)[None, :] & 1
    m = np.full((H, W), rgb[1], np.uint8)
    m[np.broadcast_to((yy == ry) & (xx == rx), (H, W))] = rgb[0]
    m[np.broadcast_to((yy != ry) & (xx != rx), (H, W))] = rgb[2]
    return m[None]


def checks():
    """The three statements of the restatement: a constant colour comes back exactly at every pixel (all patterns; 2 x 2, 3 x 2,
    24 x 34, 25 x 33); rggb / bgr equals bggr / rgb bit for bit; every value stays in [0, 255]."""
    rng = np.random.default_rng(41)
    for H, W in ((2, 2), (3, 2), (24, 34), (25, 33)):
        for pattern in PATTERNS:
            for rgb in ((200, 17, 93), (0, 255, 1), (255, 255, 255)):
                got = truth(constant_mosaic(H, W, pattern, rgb), pattern, "rgb")
                assert np.array_equal(got, np.broadcast_to(np.array(rgb, np.float32), got.shape)), (H, W, pattern, rgb)
        m = rng.integers(0, 256, (2, H, W)).astype(np.uint8)
        assert truth(m, "rggb", "bgr").tobytes() == truth(m, "bggr", "rgb").tobytes()
        assert truth(m, "grbg", "bgr").tobytes() == truth(m, "gbrg", "rgb").tobytes()
        for pattern in PATTERNS:
            t = truth(m, pattern)
            assert t.min() >= 0.0 and t.max() <= 255.0 and np.array_equal(t * 4, np.round(t * 4))
        hi = truth(np.full((1, H, W), 255, np.uint8), "grbg")
        assert hi.min() == 255.0 == hi.max()
    return True


# ----------------------------------------------------------------------------- layouts
def _packed(n, H, W):
    return dict(size=n * H * W, offset=0, strides=(H * W, W, 1), shift=(0, 0))


def _pitched(n, H, W):
    row = W + 13
    frame = H * row + 57
    return dict(size=5 + n * frame + 32, offset=5, strides=(frame, row, 1), shift=(0, 0))


def _every_second_byte(n, H, W):
    row = 2 * W + 7
    frame = H * row + 31
    return dict(size=3 + n * frame + 32, offset=3, strides=(frame, row, 2), shift=(0, 0))


def _window(n, H, W):
    """A window at row 3, column 5 of larger sensor images (H + 9) x (W + 12): the window's pattern is not the sensor's."""
    SH, SW = H + 9, W + 12
    return dict(size=n * SH * SW, offset=3 * SW + 5, strides=(SH * SW, SW, 1), shift=(3, 5))


LAYOUTS = {"packed": _packed, "pitched": _pitched, "pixel_stride_2": _every_second_byte, "odd_window": _window}


def window_pattern(pattern, y0, x0):
    """The name of the view that starts at row y0, column x0 of a mosaic named ``pattern``."""
    ry, rx = RED[pattern]
    return {v: k for k, v in RED.items()}[((ry - y0) & 1, (rx - x0) & 1)]


def spec(name, n, H, W):
    return dict(LAYOUTS[name](n, H, W), name=name, n=n, H=H, W=W)


def batch(s, seed=0):
    """Random full-range bytes [n, H, W]."""
    return np.random.default_rng(9100 + seed).integers(0, 256, (s["n"], s["H"], s["W"])).astype(np.uint8)


def view(s, parent):
    """The [n, H, W] view of the parent (NumPy; nothing copied)."""
    return np.lib.stride_tricks.as_strided(parent[s["offset"]:], (s["n"], s["H"], s["W"]), s["strides"], writeable=parent.flags.writeable)


def torch_view(s, parent):
    """The same view of a GPU parent (torch)."""
    import torch
    return torch.as_strided(parent, (s["n"], s["H"], s["W"]), s["strides"], s["offset"])


def place(s, m, fill):
    """The parent: a flat uint8 buffer filled with ``fill`` and carrying the mosaic."""
    parent = np.full(s["size"], fill, np.uint8)
    view(s, parent)[...] = m
    return parent


def span(s):
    (fs, rs, ps) = s["strides"]
    return (s["n"] - 1) * fs + (s["H"] - 1) * rs + (s["W"] - 1) * ps + 1


def struct_args(s, address, pattern, order):
    """The tuple _lib.bayer_ptr takes for the parent at ``address``."""
    (fs, rs, ps) = s["strides"]
    return (address + s["offset"], ps, rs, fs, PATTERNS.index(pattern), ORDERS.index(order))
