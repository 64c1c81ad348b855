"""The data of the planar / packed 8-bit YUV tests (tests/test_rgb_yuv.py on the GPU, tests/test_rgb_yuv_host.py without one; test
infrastructure, like tests/rgb_nv12_frames.py).

A LAYOUT says where the (Y, U, V) bytes of a batch lie: a chroma shift per axis, the sizes of one to three flat PARENTS, and per plane
(y, u, v) its parent, its byte offset inside it and its (frame, row, pixel) byte strides.  place() puts random bytes into parents
filled with one byte value (0x00, then 0xFF: a byte that is no pixel's but changes a result shows under one of the two fills) and
views() / torch_views() return the (y, u, v) triple of views.  The INDEPENDENT ORACLE is rgb_nv12_frames.convert_yuv on the bytes
gathered from the views by NumPy indexing with >> sx, >> sy (truth()).  MISTAKES are the ways a loader of this struct can go wrong,
each as the float32 frames such a loader would see."""
import numpy as np

from rgb_nv12_frames import FILLS, coefficients, convert_yuv, layout as nv12_layout  # noqa: F401  (FILLS, coefficients: re-exported)

SHIFTS = {"yuv420": (1, 1), "yuv422": (1, 0), "yuv444": (0, 0), "yuv440": (0, 1)}   # (sx, sy)


def _planar(fmt, n, H, W, order="uv", pitched=True, one_parent=False):
    """Three planes.  pitched: chroma pitch != luma pitch / 2, frame strides != rows x pitch, odd plane origins, a parent per plane;
    otherwise the planes packed one behind the other in ONE parent per frame, as a software decoder allocates them."""
    sx, sy = SHIFTS[fmt]
    ch, cw = H >> sy, W >> sx
    if pitched and not one_parent:
        yr, cr = W + 14, cw + 9
        yf, cf = H * yr + 101, ch * cr + 37
        planes = {"y": (0, 3, (yf, yr, 1)), order[0]: (1, 5, (cf, cr, 1)), order[1]: (2, 7, (cf, cr, 1))}
        return dict(fmt=fmt, sx=sx, sy=sy, sizes=[3 + n * yf + 64, 5 + n * cf + 64, 7 + n * cf + 64], **planes)
    yr, cr = (W + 6, cw + 3) if pitched else (W, cw)
    frame = H * yr + 2 * ch * cr + (11 if pitched else 0)
    planes = {"y": (0, 1, (frame, yr, 1)), order[0]: (0, 1 + H * yr, (frame, cr, 1)), order[1]: (0, 1 + H * yr + ch * cr, (frame, cr, 1))}
    return dict(fmt=fmt, sx=sx, sy=sy, sizes=[1 + n * frame + 32], **planes)


def _semi(fmt, n, H, W, order="uv", nv12_surfaces=False):
    """A luma plane and a plane of interleaved pairs (order: which byte of a pair comes first), two parents."""
    sx, sy = SHIFTS[fmt]
    ch, cw = H >> sy, W >> sx
    if nv12_surfaces:                     # exactly the surfaces of tests/rgb_nv12_frames.py (layout / place / views)
        yr, yf, cr, cf, yo, co, ys, cs = nv12_layout(n, H, W)
    else:
        yr, cr = W + 10, 2 * cw + 18
        yf, cf, yo, co = H * yr + 53, ch * cr + 29, 2, 3
        ys, cs = yo + n * yf + 64, co + n * cf + 64
    planes = {"y": (0, yo, (yf, yr, 1)), order[0]: (1, co, (cf, cr, 2)), order[1]: (1, co + 1, (cf, cr, 2))}
    return dict(fmt=fmt, sx=sx, sy=sy, sizes=[ys, cs], **planes)


def _packed422(n, H, W, offsets):
    """YUYV / UYVY: one parent, rows padded, two luma bytes and one (U, V) per four bytes."""
    row = 2 * W + 10
    frame = H * row + 21
    yo, uo, vo = offsets
    return dict(fmt="yuv422", sx=1, sy=0, sizes=[5 + n * frame + 32],
                y=(0, 5 + yo, (frame, row, 2)), u=(0, 5 + uo, (frame, row, 4)), v=(0, 5 + vo, (frame, row, 4)))


def _vuya(n, H, W):
    """Packed 4:4:4, four bytes per pixel (V, U, Y, A), rows padded."""
    row = 4 * W + 12
    frame = H * row + 8
    return dict(fmt="yuv444", sx=0, sy=0, sizes=[1 + n * frame + 32],
                y=(0, 3, (frame, row, 4)), u=(0, 2, (frame, row, 4)), v=(0, 1, (frame, row, 4)))


LAYOUTS = {
    "i420": lambda n, H, W: _planar("yuv420", n, H, W),
    "yv12": lambda n, H, W: _planar("yuv420", n, H, W, order="vu", pitched=False),
    "nv21": lambda n, H, W: _semi("yuv420", n, H, W, order="vu"),
    "nv12": lambda n, H, W: _semi("yuv420", n, H, W, nv12_surfaces=True),
    "i422": lambda n, H, W: _planar("yuv422", n, H, W, one_parent=True),
    "nv16": lambda n, H, W: _semi("yuv422", n, H, W),
    "yuyv": lambda n, H, W: _packed422(n, H, W, (0, 1, 3)),
    "uyvy": lambda n, H, W: _packed422(n, H, W, (1, 0, 2)),
    "i444": lambda n, H, W: _planar("yuv444", n, H, W),
    "vuya": lambda n, H, W: _vuya(n, H, W),
    "yuv440": lambda n, H, W: _planar("yuv440", n, H, W),          # (the C level only: no rgb_frame_format names it)
}
PYTHON_LAYOUTS = [k for k in LAYOUTS if k != "yuv440"]


def spec(name, n, H, W):
    s = LAYOUTS[name](n, H, W)
    assert H % (1 << s["sy"]) == 0 and W % (1 << s["sx"]) == 0, (name, H, W)
    return dict(s, name=name, n=n, H=H, W=W)


def batch(s, seed=0):
    """Random full-range bytes (Y [n, H, W], U and V [n, H >> sy, W >> sx])."""
    rng = np.random.default_rng(7300 + seed)
    n, H, W = s["n"], s["H"], s["W"]
    c = (n, H >> s["sy"], W >> s["sx"])
    return rng.integers(0, 256, (n, H, W)).astype(np.uint8), rng.integers(0, 256, c).astype(np.uint8), rng.integers(0, 256, c).astype(np.uint8)


def _shape(s, p):
    return (s["n"], s["H"], s["W"]) if p == "y" else (s["n"], s["H"] >> s["sy"], s["W"] >> s["sx"])


def views(s, parents):
    """The (y, u, v) views of the parents (NumPy; nothing copied)."""
    st = np.lib.stride_tricks.as_strided
    return tuple(st(parents[s[p][0]][s[p][1]:], _shape(s, p), s[p][2], writeable=parents[s[p][0]].flags.writeable) for p in "yuv")


def torch_views(s, parents):
    """The same views of GPU parents (torch)."""
    import torch
    return tuple(torch.as_strided(parents[s[p][0]], _shape(s, p), s[p][2], s[p][1]) for p in "yuv")


def place(s, Y, U, V, fill):
    """The parents: flat uint8 buffers filled with ``fill`` and carrying the three planes."""
    parents = [np.full(size, fill, np.uint8) for size in s["sizes"]]
    for view, data in zip(views(s, parents), (Y, U, V)):
        view[...] = data
    return parents


def truth(s, parents, m, oy):
    """The oracle: the bytes of every pixel gathered from the views with >> sx, >> sy, through convert_yuv."""
    y, u, v = views(s, parents)
    yy, xx = np.arange(s["H"])[:, None] >> s["sy"], np.arange(s["W"])[None, :] >> s["sx"]
    return convert_yuv(y, u[:, yy, xx], v[:, yy, xx], np.asarray(m, np.float32).reshape(3, 3), oy)


def pixel_mask(s):
    """Boolean masks over the parents: True where a byte is some pixel's Y, U or V."""
    masks = [np.zeros(size, np.uint8) for size in s["sizes"]]
    for view in views(s, masks):
        view[...] = 1
    return [m.astype(bool) for m in masks]


def struct_args(s, addresses, m, oy):
    """The tuple _lib.yuv_ptr takes for the parents at ``addresses``."""
    a = [addresses[s[p][0]] + s[p][1] for p in "yuv"]
    assert s["u"][2] == s["v"][2]
    (yf, yr, yp), (cf, cr, cp) = s["y"][2], s["u"][2]
    return tuple(a) + (yp, yr, yf, cp, cr, cf, s["sx"], s["sy"], [float(c) for c in np.asarray(m, np.float32).reshape(9)], float(oy))


# ----------------------------------------------------------------------------- the mistakes a loader of this struct can make
# Each: the float32 frames [n, H, W, 3] a kernel with that mistake would see on the parents; an address past a parent wraps into it
# (what lies there is somebody else's memory).

def see(s, parents, m, oy, **wrong):
    """wrong: sx / sy (the shift a wrong loader applies), cp / cr / cf / yp (a stride it takes), swap (U <-> V), v_through_u."""
    (yf, yr, yp), (cf, cr, cp) = s["y"][2], s["u"][2]
    yp, cp, cr, cf = (wrong.get(k, d) for k, d in (("yp", yp), ("cp", cp), ("cr", cr), ("cf", cf)))
    sx, sy = wrong.get("sx", s["sx"]), wrong.get("sy", s["sy"])
    f, y, x = np.meshgrid(np.arange(s["n"]), np.arange(s["H"]), np.arange(s["W"]), indexing="ij")
    c = f * cf + (y >> sy) * cr + (x >> sx) * cp

    def take(p, off):
        parent = parents[s[p][0]]
        return np.take(parent, (s[p][1] + off) % parent.size)

    Y, U, V = take("y", f * yf + y * yr + x * yp), take("u", c), take("u" if wrong.get("v_through_u") else "v", c)
    if wrong.get("swap"):
        U, V = V, U
    return convert_yuv(Y, U, V, np.asarray(m, np.float32).reshape(3, 3), oy)


# name -> (applies to a layout?, the keywords of see())
MISTAKES = {
    "chroma_shift_x not applied": (lambda s: s["sx"] == 1, lambda s: dict(sx=0)),
    "chroma_shift_y not applied": (lambda s: s["sy"] == 1, lambda s: dict(sy=0)),
    "the luma pixel stride used for chroma": (lambda s: s["y"][2][2] != s["u"][2][2], lambda s: dict(cp=s["y"][2][2])),
    "the chroma pixel stride used for luma": (lambda s: s["y"][2][2] != s["u"][2][2], lambda s: dict(yp=s["u"][2][2])),
    "U and V swapped": (lambda s: True, lambda s: dict(swap=True)),
    "V read through U's pointer": (lambda s: True, lambda s: dict(v_through_u=True)),
    "the chroma row stride taken as luma's": (lambda s: s["y"][2][1] != s["u"][2][1], lambda s: dict(cr=s["y"][2][1])),
    "the chroma frame stride taken as luma's": (lambda s: s["y"][2][0] != s["u"][2][0], lambda s: dict(cf=s["y"][2][0])),
}
