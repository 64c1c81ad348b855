"""The data of the NV12 tests (tests/test_rgb_nv12.py on the GPU, tests/test_rgb_nv12_host.py without one; test infrastructure, like
tests/rgb_uint8_frames.py and tests/rgb_strided_views.py).

convert() is the INDEPENDENT ORACLE of the conversion include/silent_hip.h specifies: a NumPy restatement with separate np.float32
multiplies and adds in the header's order.  coefficients() restates the closed forms of the matrices.  A LAYOUT places a batch of
(Y, U, V) bytes into two flat parents -- luma and chroma, with different pitches and frame strides -- filled with one byte value
(0x00 or 0xFF: a byte that is not a pixel's but changes a result shows under one of the two fills).  MISTAKES are the ways an NV12
loader can go wrong, each as the float32 frames such a loader would see."""
import hashlib

import numpy as np

FILLS = (0x00, 0xFF)
MATRICES = {"bt601": (.299, .114), "bt709": (.2126, .0722)}
VARIANTS = [(mx, rg, od) for mx in ("bt601", "bt709") for rg in ("limited", "full") for od in ("bgr", "rgb")]


def coefficients(matrix, rng, order):
    """(m [3, 3] float32, oy float32) from the closed forms, in float64, each coefficient rounded once."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs, oy = (255.0 / 219.0, 255.0 / 224.0, 16.0) if rng == "limited" else (1.0, 1.0, 0.0)
    r = [ys, 0.0, 2.0 * (1.0 - kr) * cs]
    g = [ys, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs]
    b = [ys, 2.0 * (1.0 - kb) * cs, 0.0]
    rows = [b, g, r] if order == "bgr" else [r, g, b]
    return np.array(rows, np.float64).astype(np.float32), np.float32(oy)


def convert(y, uv, m, oy, clamp=True):
    """y [n, H, W] uint8, uv [n, H / 2, W / 2, 2] uint8 -> [n, H, W, 3] float32: every product and every sum a separately rounded
    float32 operation, nearest chroma, clamped to [0, 255], not rounded to an integer."""
    m = np.asarray(m, np.float32).reshape(3, 3)
    n, H, W = y.shape
    yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    return convert_yuv(y, uv[:, yy, xx, 0], uv[:, yy, xx, 1], m, oy, clamp)


def convert_yuv(Y, U, V, m, oy, clamp=True):
    """The same on per-pixel bytes Y, U, V of one shape."""
    f = np.float32
    yv = Y.astype(f) - f(oy)
    uvv = U.astype(f) - f(128)
    vv = V.astype(f) - f(128)
    out = np.empty(Y.shape + (3,), f)
    for k in range(3):
        a = (yv * f(m[k, 0])).astype(f)
        b = (uvv * f(m[k, 1])).astype(f)
        c = (vv * f(m[k, 2])).astype(f)
        s = ((a + b).astype(f) + c).astype(f)
        out[..., k] = np.minimum(np.maximum(s, f(0)), f(255)) if clamp else s
    return out


def batch(n, H, W, seed=0):
    """Random full-range bytes: (y [n, H, W], uv [n, H / 2, W / 2, 2])."""
    rng = np.random.default_rng(4100 + seed)
    return rng.integers(0, 256, (n, H, W)).astype(np.uint8), rng.integers(0, 256, (n, H // 2, W // 2, 2)).astype(np.uint8)


def combinations():
    """One 256 x 256 frame that holds every one of the 256 Y values with every (U, V) of a 16 x 16 grid (0, 17, ..., 255 each): chroma
    block b = 128 by + bx carries combination b % 256, and its four pixels the Y values 4 (b // 256) + 0 .. 3."""
    by, bx = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    b = by * 128 + bx
    uv = np.stack([(b % 256) // 16 * 17, (b % 256) % 16 * 17], -1).astype(np.uint8)[None]
    yy, xx = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    y = (4 * (((yy >> 1) * 128 + (xx >> 1)) // 256) + 2 * (yy & 1) + (xx & 1)).astype(np.uint8)[None]
    return y, uv


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


# ----------------------------------------------------------------------------- layouts

def layout(n, H, W):
    """Byte strides of the test surfaces: (y_row, y_frame, uv_row, uv_frame, y offset, uv offset, y parent size, uv parent size) --
    the chroma pitch differs from the luma pitch, neither frame stride is rows x pitch, the chroma plane starts at an odd byte."""
    yr, ur = W + 14, W + 30
    yf, uf = H * yr + 101, (H // 2) * ur + 37
    return yr, yf, ur, uf, 3, 5, 3 + n * yf + 64, 5 + n * uf + 64


def place(y, uv, fill):
    """(luma parent, chroma parent): flat uint8 buffers filled with ``fill`` and carrying the planes through layout()."""
    n, H, W = y.shape
    yr, yf, ur, uf, yo, uo, ys, us = layout(n, H, W)
    py, pu = np.full(ys, fill, np.uint8), np.full(us, fill, np.uint8)
    views(py, pu, n, H, W)[0][...] = y
    views(py, pu, n, H, W)[1][...] = uv
    return py, pu


def views(py, pu, n, H, W):
    """The (y, uv) views of the two parents (NumPy; nothing copied)."""
    yr, yf, ur, uf, yo, uo, _, _ = layout(n, H, W)
    st = np.lib.stride_tricks.as_strided
    return (st(py[yo:], (n, H, W), (yf, yr, 1), writeable=py.flags.writeable),
            st(pu[uo:], (n, H // 2, W // 2, 2), (uf, ur, 2, 1), writeable=pu.flags.writeable))


def torch_views(py, pu, n, H, W):
    """The same views of two GPU parents (torch)."""
    import torch
    yr, yf, ur, uf, yo, uo, _, _ = layout(n, H, W)
    return (torch.as_strided(py, (n, H, W), (yf, yr, 1), yo), torch.as_strided(pu, (n, H // 2, W // 2, 2), (uf, ur, 2, 1), uo))


def pixel_mask(n, H, W):
    """Boolean masks over the two parents: True where a byte is a pixel's Y or part of a pixel's (U, V) pair."""
    _, _, _, _, _, _, ys, us = layout(n, H, W)
    my, mu = np.zeros(ys, np.uint8), np.zeros(us, np.uint8)
    a, b = views(my, mu, n, H, W)
    a[...] = 1
    b[...] = 1
    return my.astype(bool), mu.astype(bool)


# ----------------------------------------------------------------------------- the mistakes an NV12 loader can make
# Each: the float32 frames [n, H, W, 3] a kernel with that mistake would see on the two parents; an address past a parent wraps into
# it (what lies there is somebody else's memory).

def _see(py, pu, n, H, W, m, oy, swap=False, crow=lambda y: y >> 1, ccol=lambda x: x >> 1, ur=None, uf=None, clamp=True):
    yr, yf, ur0, uf0, yo, uo, _, _ = layout(n, H, W)
    ur, uf = ur0 if ur is None else ur, uf0 if uf is None else uf
    f, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
    Y = np.take(py, (yo + f * yf + y * yr + x) % py.size)
    c = uo + f * uf + crow(y) * ur + 2 * ccol(x)
    U, V = np.take(pu, c % pu.size), np.take(pu, (c + 1) % pu.size)
    if swap:
        U, V = V, U
    return convert_yuv(Y, U, V, np.asarray(m, np.float32).reshape(3, 3), oy, clamp)


def truth(py, pu, n, H, W, m, oy):
    return _see(py, pu, n, H, W, m, oy)


MISTAKES = {
    "U and V swapped": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, oy, swap=True),
    "chroma row y instead of y >> 1": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, oy, crow=lambda y: y),
    "chroma column x instead of x >> 1": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, oy, ccol=lambda x: x),
    "the Y pitch used for UV": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, oy, ur=layout(n, H, W)[0]),
    "the UV frame stride taken as Y's": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, oy, uf=layout(n, H, W)[1]),
    "oy dropped": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, 0.0),
    "m transposed": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, np.asarray(m, np.float32).reshape(3, 3).T, oy),
    "clamp missing": lambda py, pu, n, H, W, m, oy: _see(py, pu, n, H, W, m, oy, clamp=False),
}
# the frames on which a mistake acts (the frame stride: frame 1 only)
FRAMES_HIT = {"the UV frame stride taken as Y's": (1,)}
