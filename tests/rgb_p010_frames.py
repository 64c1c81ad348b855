"""The data of the P010 / P012 / P016 tests (tests/test_rgb_p010.py on the GPU, tests/test_rgb_p010_host.py without one; test
infrastructure, like tests/rgb_nv12_frames.py).

convert() is the INDEPENDENT ORACLE of the conversion include/silent_hip.h specifies: a NumPy restatement with separate np.float32
subtractions, multiplies and adds in the header's order on unsigned elements shifted right by 16 - depth.  coefficients() restates the
closed forms of the matrices.  A LAYOUT places a batch of uint16 (Y, U, V) elements into two flat uint16 parents -- luma and chroma,
with different pitches and frame strides, the chroma plane starting at an address that is 2 (mod 4) -- filled with one byte value
(0x00 or 0xFF: a byte that is not a pixel's but changes a result shows under one of the two fills).  MISTAKES are the ways a P010 loader
can go wrong, each as the float32 frames such a loader would see."""
import hashlib

import numpy as np

FILLS = (0x00, 0xFF)
DEPTHS = (10, 12, 16)
MATRICES = {"bt601": (.299, .114), "bt709": (.2126, .0722), "bt2020": (.2627, .0593)}
VARIANTS = [(mx, rg, od) for mx in ("bt601", "bt709", "bt2020") for rg in ("limited", "full") for od in ("bgr", "rgb")]


def coefficients(matrix, rng, order, depth):
    """(m [3, 3] float32, oy float32, oc float32) from the closed forms, in float64, each coefficient rounded once."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    s = 2.0 ** (depth - 8)
    if rng == "limited":
        ys, cs, oy = 255.0 / (219.0 * s), 255.0 / (224.0 * s), 16.0 * s
    else:
        ys = cs = 255.0 / (2.0 ** depth - 1.0)
        oy = 0.0
    r = [ys, 0.0, 2.0 * (1.0 - kr) * cs]
    g = [ys, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs]
    b = [ys, 2.0 * (1.0 - kb) * cs, 0.0]
    rows = [b, g, r] if order == "bgr" else [r, g, b]
    return np.array(rows, np.float64).astype(np.float32), np.float32(oy), np.float32(128.0 * s)


def convert(y, uv, m, oy, oc, shift, clamp=True):
    """y [n, H, W] uint16, uv [n, H / 2, W / 2, 2] uint16 -> [n, H, W, 3] float32: the code is the element >> shift (unsigned), every
    difference, product and sum a separately rounded float32 operation, nearest chroma, clamped to [0, 255], not rounded to an integer."""
    n, H, W = y.shape
    yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    return convert_yuv(y, uv[:, yy, xx, 0], uv[:, yy, xx, 1], m, oy, oc, shift, clamp)


def convert_codes(Yc, Uc, Vc, m, oy, oc, clamp=True):
    """The arithmetic on per-pixel CODES (any integer or float array that float32 holds exactly)."""
    f = np.float32
    m = np.asarray(m, f).reshape(3, 3)
    yv = (Yc.astype(f) - f(oy)).astype(f)
    uvv = (Uc.astype(f) - f(oc)).astype(f)
    vv = (Vc.astype(f) - f(oc)).astype(f)
    out = np.empty(Yc.shape + (3,), f)
    for k in range(3):
        a = (yv * f(m[k, 0])).astype(f)
        b = (uvv * f(m[k, 1])).astype(f)
        c = (vv * f(m[k, 2])).astype(f)
        s = ((a + b).astype(f) + c).astype(f)
        out[..., k] = np.minimum(np.maximum(s, f(0)), f(255)) if clamp else s
    return out


def convert_yuv(Y, U, V, m, oy, oc, shift, clamp=True):
    """The same on per-pixel uint16 ELEMENTS Y, U, V of one shape."""
    assert Y.dtype == np.uint16 and U.dtype == np.uint16 and V.dtype == np.uint16
    sh = np.uint32(shift)
    return convert_codes(Y.astype(np.uint32) >> sh, U.astype(np.uint32) >> sh, V.astype(np.uint32) >> sh, m, oy, oc, clamp)


def elements(codes, depth, rng):
    """Codes of ``depth`` bits as uint16 elements: the code in the high bits, RANDOM low bits (decoders do not promise zeros)."""
    shift = 16 - depth
    junk = rng.integers(0, 1 << shift, codes.shape) if shift else 0
    return ((codes.astype(np.int64) << shift) | junk).astype(np.uint16)


def batch(n, H, W, depth=10, seed=0):
    """Random full-range codes with random low bits: (y [n, H, W], uv [n, H / 2, W / 2, 2]) uint16."""
    rng = np.random.default_rng(9100 + seed)
    return (elements(rng.integers(0, 1 << depth, (n, H, W)), depth, rng), elements(rng.integers(0, 1 << depth, (n, H // 2, W // 2, 2)), depth, rng))


GRID10 = (0, 146, 292, 438, 512, 658, 877, 1023)


def combinations10():
    """One 256 x 256 P010 frame that holds every one of the 1024 luma codes with every (U, V) of an 8 x 8 grid (GRID10, which has 0,
    512 and 1023): chroma block b = 128 by + bx carries combination b % 64, and its four pixels the luma codes 4 (b // 64) + 0 .. 3.
    Random low bits."""
    rng = np.random.default_rng(9010)
    by, bx = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    b = by * 128 + bx
    g = np.array(GRID10)
    uv = np.stack([g[(b % 64) // 8], g[(b % 64) % 8]], -1)[None]
    yy, xx = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    y = (4 * (((yy >> 1) * 128 + (xx >> 1)) // 64) + 2 * (yy & 1) + (xx & 1))[None]
    return elements(y, 10, rng), elements(uv, 10, rng)


def special_codes(depth):
    s = 1 << (depth - 8)
    return (0, 1, 16 * s - 1, 16 * s, 16 * s + 1, 1 << (depth - 1), (1 << depth) - 2, (1 << depth) - 1)


def extremes(depth):
    """One 32 x 32 frame: the codes {0, 1, oy - 1, oy, oy + 1, half, max - 1, max} (oy = 16 s) in the luma of the upper half and as every
    (U, V) pair of the upper chroma rows, random codes below; random low bits."""
    rng = np.random.default_rng(9000 + depth)
    sp = np.array(special_codes(depth))
    y = rng.integers(0, 1 << depth, (1, 32, 32))
    uv = rng.integers(0, 1 << depth, (1, 16, 16, 2))
    y[0, :16] = sp[(np.arange(32)[None, :] + np.arange(16)[:, None]) % 8]
    uv[0, :8, :, 0] = sp[np.arange(8)][:, None]
    uv[0, :8, :, 1] = sp[np.arange(16) % 8][None, :]
    return elements(y, depth, rng), elements(uv, depth, rng)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


# ----------------------------------------------------------------------------- layouts

def layout(n, H, W):
    """ELEMENT strides of the test surfaces: (y_row, y_frame, uv_row, uv_frame, y offset, uv offset, y parent size, uv parent size) --
    the chroma pitch differs from the luma pitch, neither frame stride is rows x pitch, the chroma plane starts at an odd element (an
    address that is 2 mod 4 in a 4-byte aligned parent) and its pitch is odd, so the pairs of consecutive chroma rows alternate
    between addresses that are 2 and 0 (mod 4)."""
    yr, ur = W + 7, W + 15
    yf, uf = H * yr + 51, (H // 2) * ur + 19
    return yr, yf, ur, uf, 3, 5, 3 + n * yf + 32, 5 + n * uf + 32


def place(y, uv, fill):
    """(luma parent, chroma parent): flat uint16 buffers whose BYTES are ``fill`` and that carry the planes through layout()."""
    n, H, W = y.shape
    yr, yf, ur, uf, yo, uo, ys, us = layout(n, H, W)
    py, pu = np.full(ys, fill * 0x0101, np.uint16), np.full(us, fill * 0x0101, np.uint16)
    views(py, pu, n, H, W)[0][...] = y
    views(py, pu, n, H, W)[1][...] = uv
    return py, pu


def views(py, pu, n, H, W):
    """The (y, uv) views of the two parents (NumPy; nothing copied)."""
    yr, yf, ur, uf, yo, uo, _, _ = layout(n, H, W)
    st = np.lib.stride_tricks.as_strided
    return (st(py[yo:], (n, H, W), (2 * yf, 2 * yr, 2), writeable=py.flags.writeable),
            st(pu[uo:], (n, H // 2, W // 2, 2), (2 * uf, 2 * ur, 4, 2), writeable=pu.flags.writeable))


def torch_views(py, pu, n, H, W):
    """The same views of two GPU parents (torch.uint16)."""
    import torch
    yr, yf, ur, uf, yo, uo, _, _ = layout(n, H, W)
    return (torch.as_strided(py, (n, H, W), (yf, yr, 1), yo), torch.as_strided(pu, (n, H // 2, W // 2, 2), (uf, ur, 2, 1), uo))


def pixel_mask(n, H, W):
    """Boolean masks over the ELEMENTS of the two parents: True where an element is a pixel's Y or part of a pixel's (U, V) pair."""
    _, _, _, _, _, _, ys, us = layout(n, H, W)
    my, mu = np.zeros(ys, np.uint16), np.zeros(us, np.uint16)
    a, b = views(my, mu, n, H, W)
    a[...] = 1
    b[...] = 1
    return my.astype(bool), mu.astype(bool)


# ----------------------------------------------------------------------------- the mistakes a P010 loader can make
# Each: the float32 frames [n, H, W, 3] a kernel with that mistake would see on the two parents, addressed by BYTES (little-endian
# elements); an address past a parent wraps into it (what lies there is somebody else's memory).

def _see(py, pu, n, H, W, m, oy, oc, shift, swap=False, crow=lambda y: y >> 1, ccol=lambda x: x >> 1, ur=None, uf=None, clamp=True,
         signed=False, v_at=2, stride_scale=1, drop_shift=False):
    yr, yf, ur0, uf0, yo, uo, _, _ = layout(n, H, W)
    ur, uf = ur0 if ur is None else ur, uf0 if uf is None else uf
    by, bu = py.view(np.uint8), pu.view(np.uint8)
    k = 2 * stride_scale                              # bytes per element stride unit

    def element(parent, a):
        return np.take(parent, a % parent.size).astype(np.int64) | (np.take(parent, (a + 1) % parent.size).astype(np.int64) << 8)

    f, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
    Y = element(by, 2 * yo + k * (f * yf + y * yr) + 2 * x)
    c = 2 * uo + k * (f * uf + crow(y) * ur) + 4 * ccol(x)
    U, V = element(bu, c), element(bu, c + v_at)
    if swap:
        U, V = V, U
    if signed:
        Y, U, V = (np.where(e >= 0x8000, e - 0x10000, e) for e in (Y, U, V))
    sh = 0 if drop_shift else shift
    return convert_codes(Y >> sh, U >> sh, V >> sh, m, oy, oc, clamp)


def truth(py, pu, n, H, W, m, oy, oc, shift):
    return _see(py, pu, n, H, W, m, oy, oc, shift)


def _mistake(**kw):
    return lambda py, pu, n, H, W, m, oy, oc, shift: _see(py, pu, n, H, W, m, oy, oc, shift, **kw)


MISTAKES = {
    "U and V swapped": _mistake(swap=True),
    "chroma row y instead of y >> 1": _mistake(crow=lambda y: y),
    "chroma column x instead of x >> 1": _mistake(ccol=lambda x: x),
    "the Y pitch used for UV": lambda py, pu, n, H, W, m, oy, oc, shift: _see(py, pu, n, H, W, m, oy, oc, shift, ur=layout(n, H, W)[0]),
    "the UV frame stride taken as Y's": lambda py, pu, n, H, W, m, oy, oc, shift: _see(py, pu, n, H, W, m, oy, oc, shift, uf=layout(n, H, W)[1]),
    "oy dropped": lambda py, pu, n, H, W, m, oy, oc, shift: _see(py, pu, n, H, W, m, 0.0, oc, shift),
    "m transposed": lambda py, pu, n, H, W, m, oy, oc, shift: _see(py, pu, n, H, W, np.asarray(m, np.float32).reshape(3, 3).T, oy, oc, shift),
    "clamp missing": _mistake(clamp=False),
    "the shift dropped": _mistake(drop_shift=True),
    "oc = 128 instead of 128 s": lambda py, pu, n, H, W, m, oy, oc, shift: _see(py, pu, n, H, W, m, oy, 128.0, shift),
    "the element loaded signed": _mistake(signed=True),
    "V one byte after U": _mistake(v_at=1),
    "byte strides taken as element strides": _mistake(stride_scale=2),
}
# the frames on which a mistake acts (the frame stride: frame 1 only)
FRAMES_HIT = {"the UV frame stride taken as Y's": (1,)}
