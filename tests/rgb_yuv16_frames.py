"""The data of the 16-bit planar / semi-planar / packed YUV tests (tests/test_rgb_yuv16.py on the GPU, tests/test_rgb_yuv16_host.py
without one; test infrastructure, like tests/rgb_yuv_frames.py and tests/rgb_p010_frames.py).

A LAYOUT says where the (Y, U, V) ELEMENTS of a batch lie: a chroma shift per axis, where the code sits (depth, shift), the sizes of
one to three flat uint16 PARENTS, and per plane (y, u, v) its parent, its ELEMENT offset inside it and its (frame, row, pixel) ELEMENT
strides (the struct takes bytes: twice these).  place() puts the elements into parents whose BYTES are one value (0x00, then 0xFF: a
byte that is no pixel's but changes a result shows under one of the two fills); views() / torch_views() return the (y, u, v) triple.
The INDEPENDENT ORACLE is convert(): a NumPy gather with >> sx, >> sy, then shift and mask, then separately rounded float32
operations (truth()).  MISTAKES are the ways a loader of this struct can go wrong, each as the float32 frames such a loader would see."""
import hashlib

import numpy as np

FILLS = (0x00, 0xFF)
SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "440": (0, 1)}   # (sx, sy)


def fmt_name(sub, depth, shift):
    """The rgb_frame_format of a (subsampling, depth, shift), None where Python has no name (4:4:0, depths 9 / 14 ...)."""
    if sub == "440" or depth not in (10, 12, 16) or shift not in (0, 16 - depth):
        return None
    return "yuv%sp%d%s" % (sub, depth, "msb" if shift and depth != 16 else "")


def codes_of(e, shift, depth):
    """code(e) = (e >> shift) & ((1 << depth) - 1) on UNSIGNED elements."""
    return (np.asarray(e).astype(np.uint32) >> np.uint32(shift)) & np.uint32((1 << depth) - 1)


def convert_codes(Yc, Uc, Vc, m, oy, oc):
    """Per-pixel codes -> [..., 3] float32: every difference, product and sum one float32 operation, clamped to [0, 255]."""
    f = np.float32
    m = np.asarray(m, f).reshape(3, 3)
    yv, uv, vv = (Yc.astype(f) - f(oy)).astype(f), (Uc.astype(f) - f(oc)).astype(f), (Vc.astype(f) - f(oc)).astype(f)
    out = np.empty(Yc.shape + (3,), f)
    for k in range(3):
        a, b, c = (yv * m[k, 0]).astype(f), (uv * m[k, 1]).astype(f), (vv * m[k, 2]).astype(f)
        out[..., k] = np.minimum(np.maximum(((a + b).astype(f) + c).astype(f), f(0)), f(255))
    return out


def convert(y, u, v, sx, sy, m, oy, oc, shift, depth):
    """THE restatement: y [n, H, W], u and v [n, H >> sy, W >> sx] uint16 -> [n, H, W, 3] float32."""
    assert y.dtype == u.dtype == v.dtype == np.uint16
    H, W = y.shape[1:]
    yy, xx = np.arange(H)[:, None] >> sy, np.arange(W)[None, :] >> sx
    return convert_codes(codes_of(y, shift, depth), codes_of(u[:, yy, xx], shift, depth), codes_of(v[:, yy, xx], shift, depth), m, oy, oc)


def coefficients(matrix="bt709", rng="limited", order="bgr", depth=10):
    from rgb_p010_frames import coefficients as c
    return c(matrix, rng, order, depth)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


# ----------------------------------------------------------------------------- layouts (ELEMENT units)

def _planar(sub, depth, n, H, W, one_parent=False, shift=0):
    """Three planes, the code in the low bits.  Row strides are ODD element counts (no multiple of 4 bytes), plane origins odd
    elements (addresses that are 2 mod 4), the chroma pitch unrelated to the luma pitch, frame strides not rows x pitch."""
    sx, sy = SHIFTS[sub]
    ch, cw = H >> sy, W >> sx
    if not one_parent:
        yr, cr = (W + 7) | 1, (cw + 10) | 1
        yf, cf = H * yr + 51, ch * cr + 18
        return dict(sub=sub, sx=sx, sy=sy, depth=depth, shift=shift, sizes=[3 + n * yf + 32, 5 + n * cf + 32, 7 + n * cf + 32],
                    y=(0, 3, (yf, yr, 1)), u=(1, 5, (cf, cr, 1)), v=(2, 7, (cf, cr, 1)))
    yr, cr = (W + 4) | 1, (cw + 2) | 1                  # as a software decoder allocates a frame: one block, the planes in a row
    frame = H * yr + 2 * ch * cr + 11
    return dict(sub=sub, sx=sx, sy=sy, depth=depth, shift=shift, sizes=[1 + n * frame + 16],
                y=(0, 1, (frame, yr, 1)), u=(0, 1 + H * yr, (frame, cr, 1)), v=(0, 1 + H * yr + ch * cr, (frame, cr, 1)))


def _semi(sub, depth, n, H, W, order="uv", p010_surfaces=False):
    """A luma plane and a plane of interleaved element pairs, the code in the high bits (shift = 16 - depth), two parents."""
    sx, sy = SHIFTS[sub]
    ch, cw = H >> sy, W >> sx
    if p010_surfaces:                     # exactly the surfaces of tests/rgb_p010_frames.py (layout / place / views)
        from rgb_p010_frames import layout as p010_layout
        yr, yf, cr, cf, yo, co, ys, cs = p010_layout(n, H, W)
    else:
        yr, cr = (W + 8) | 1, (2 * cw + 12) | 1
        yf, cf, yo, co = H * yr + 53, ch * cr + 29, 1, 3
        ys, cs = yo + n * yf + 32, co + n * cf + 32
    planes = {"y": (0, yo, (yf, yr, 1)), order[0]: (1, co, (cf, cr, 2)), order[1]: (1, co + 1, (cf, cr, 2))}
    return dict(sub=sub, sx=sx, sy=sy, depth=depth, shift=16 - depth, sizes=[ys, cs], **planes)


def _y210(depth, n, H, W):
    """Y210 / Y216: one parent, rows padded, Y0 U Y1 V elements."""
    row = (2 * W + 10) | 1
    frame = H * row + 21
    return dict(sub="422", sx=1, sy=0, depth=depth, shift=16 - depth, sizes=[3 + n * frame + 16],
                y=(0, 3, (frame, row, 2)), u=(0, 4, (frame, row, 4)), v=(0, 6, (frame, row, 4)))


def _y416(n, H, W):
    """Y416: packed 4:4:4, four elements per pixel (U, Y, V, A), rows padded."""
    row = (4 * W + 12) | 1
    frame = H * row + 8
    return dict(sub="444", sx=0, sy=0, depth=16, shift=0, sizes=[1 + n * frame + 16],
                y=(0, 2, (frame, row, 4)), u=(0, 1, (frame, row, 4)), v=(0, 3, (frame, row, 4)))


LAYOUTS = {
    "i010": lambda n, H, W: _planar("420", 10, n, H, W),
    "i012": lambda n, H, W: _planar("420", 12, n, H, W, one_parent=True),
    "i016": lambda n, H, W: _planar("420", 16, n, H, W),
    "p010": lambda n, H, W: _semi("420", 10, n, H, W, p010_surfaces=True),
    "vu010": lambda n, H, W: _semi("420", 10, n, H, W, order="vu"),
    "i210": lambda n, H, W: _planar("422", 10, n, H, W, one_parent=True),
    "p210": lambda n, H, W: _semi("422", 10, n, H, W),
    "p212": lambda n, H, W: _semi("422", 12, n, H, W),
    "p216": lambda n, H, W: _semi("422", 16, n, H, W),
    "y210": lambda n, H, W: _y210(10, n, H, W),
    "y216": lambda n, H, W: _y210(16, n, H, W),
    "i410": lambda n, H, W: _planar("444", 10, n, H, W),
    "i412": lambda n, H, W: _planar("444", 12, n, H, W),
    "p410": lambda n, H, W: _semi("444", 10, n, H, W),
    "y416": lambda n, H, W: _y416(n, H, W),
    "yuv440": lambda n, H, W: _planar("440", 10, n, H, W),           # (the C level only: no rgb_frame_format names it)
    "i009": lambda n, H, W: _planar("420", 9, n, H, W),              # (the C level only: depth 9, low bits)
    "m014": lambda n, H, W: _planar("422", 14, n, H, W, shift=1),    # (the C level only: depth 14 in bits 1 .. 14)
}
PYTHON_LAYOUTS = [k for k in LAYOUTS if k not in ("yuv440", "i009", "m014")]


def spec(name, n, H, W):
    s = LAYOUTS[name](n, H, W)
    assert H % (1 << s["sy"]) == 0 and W % (1 << s["sx"]) == 0, (name, H, W)
    return dict(s, name=name, n=n, H=H, W=W, fmt=fmt_name(s["sub"], s["depth"], s["shift"]))


def elements(codes, shift, depth, rng):
    """Codes as uint16 elements with RANDOM bits everywhere outside [shift, shift + depth)."""
    outside = 0xFFFF & ~(((1 << depth) - 1) << shift)
    return ((codes.astype(np.int64) << shift) | (rng.integers(0, 1 << 16, codes.shape) & outside)).astype(np.uint16)


def batch(s, seed=0, junk=True):
    """Random full-range codes (Y [n, H, W], U and V [n, H >> sy, W >> sx]) as elements; junk: random bits outside the code."""
    rng, other = np.random.default_rng(7600 + seed), np.random.default_rng(8600 + seed)   # (the codes do not depend on ``junk``)
    n, H, W = s["n"], s["H"], s["W"]
    c = (n, H >> s["sy"], W >> s["sx"])
    out = []
    for shape in ((n, H, W), c, c):
        codes = rng.integers(0, 1 << s["depth"], shape)
        out.append(elements(codes, s["shift"], s["depth"], other) if junk else (codes << s["shift"]).astype(np.uint16))
    return tuple(out)


def _shape(s, p):
    return (s["n"], s["H"], s["W"]) if p == "y" else (s["n"], s["H"] >> s["sy"], s["W"] >> s["sx"])


def views(s, parents):
    """The (y, u, v) views of the parents (NumPy; nothing copied)."""
    st = np.lib.stride_tricks.as_strided
    return tuple(st(parents[s[p][0]][s[p][1]:], _shape(s, p), tuple(2 * e for e in s[p][2]), writeable=parents[s[p][0]].flags.writeable)
                 for p in "yuv")


def torch_views(s, parents):
    """The same views of GPU parents (torch.uint16)."""
    import torch
    return tuple(torch.as_strided(parents[s[p][0]], _shape(s, p), s[p][2], s[p][1]) for p in "yuv")


def place(s, Y, U, V, fill):
    """The parents: flat uint16 buffers whose BYTES are ``fill`` and that carry the three planes."""
    parents = [np.full(size, fill * 0x0101, np.uint16) for size in s["sizes"]]
    for view, data in zip(views(s, parents), (Y, U, V)):
        view[...] = data
    return parents


def truth(s, parents, m, oy, oc):
    y, u, v = views(s, parents)
    return convert(y, u, v, s["sx"], s["sy"], m, oy, oc, s["shift"], s["depth"])


def pixel_mask(s):
    """Boolean masks over the ELEMENTS of the parents: True where an element is some pixel's Y, U or V."""
    masks = [np.zeros(size, np.uint16) for size in s["sizes"]]
    for view in views(s, masks):
        view[...] = 1
    return [m.astype(bool) for m in masks]


def struct_args(s, addresses, m, oy, oc):
    """The tuple _lib.yuv16_ptr takes for the parents at ``addresses`` (bytes)."""
    a = [addresses[s[p][0]] + 2 * s[p][1] for p in "yuv"]
    assert s["u"][2] == s["v"][2]
    (yf, yr, yp), (cf, cr, cp) = s["y"][2], s["u"][2]
    return tuple(a) + (2 * yp, 2 * yr, 2 * yf, 2 * cp, 2 * cr, 2 * cf, s["sx"], s["sy"],
                       [float(c) for c in np.asarray(m, np.float32).reshape(9)], float(oy), float(oc), s["shift"], s["depth"])


# ----------------------------------------------------------------------------- the mistakes a loader of this struct can make
# Each: the float32 frames [n, H, W, 3] a kernel with that mistake would see on the parents, addressed by BYTES (little-endian
# elements); an address outside a parent wraps into it (what lies there is somebody else's memory).

def see(s, parents, m, oy, oc, **wrong):
    """wrong: signed (the element sign-extended, and the mask -- redundant for a high-aligned code -- left out where shift + depth ==
    16: with the mask a sign extension cannot show), no_mask, no_shift, scale (byte strides taken as element strides: 2), swap (U <->
    V), swap_shifts (sx <-> sy), cr (a chroma row stride, elements), frame32 (the chroma frame term wrapped to 32 bits, with the chroma
    frames that many bytes apart: see below), oc_used (the chroma offset taken)."""
    (yf, yr, yp), (cf, cr, cp) = s["y"][2], s["u"][2]
    cr = wrong.get("cr", cr)
    sx, sy = (s["sy"], s["sx"]) if wrong.get("swap_shifts") else (s["sx"], s["sy"])
    k = 2 * wrong.get("scale", 1)
    f, y, x = np.meshgrid(np.arange(s["n"]), np.arange(s["H"]), np.arange(s["W"]), indexing="ij")
    bytes_of = [p.view(np.uint8) for p in parents]

    def element(p, off):
        b = bytes_of[s[p][0]]
        a = 2 * s[p][1] + off
        return np.take(b, a % b.size).astype(np.int64) | (np.take(b, (a + 1) % b.size).astype(np.int64) << 8)

    fterm = f * cf * k
    if "frame32" in wrong:
        # the chroma frames as if they lay virtual_cf bytes apart (2^31 + 4098): the right loader's 64-bit term reaches frame f, a
        # 32-bit term wraps to a negative offset for f = 1 -- memory in front of the plane, here the parent wrapped around
        virtual = f.astype(np.int64) * wrong["frame32"]
        wrapped = ((virtual + 2 ** 31) % 2 ** 32) - 2 ** 31
        fterm = np.where(wrapped == virtual, fterm, wrapped)
    c = fterm + k * ((y >> sy) * cr) + (x >> sx) * 2 * cp
    Y, U, V = element("y", k * (f * yf + y * yr) + x * 2 * yp), element("u", c), element("v", c)
    if wrong.get("swap"):
        U, V = V, U
    shift, mask = (0 if wrong.get("no_shift") else s["shift"]), (1 << s["depth"]) - 1
    if wrong.get("signed"):
        Y, U, V = (np.where(e >= 0x8000, e - 0x10000, e) for e in (Y, U, V))
        if s["shift"] + s["depth"] == 16:
            mask = -1
    if wrong.get("no_mask"):
        mask = -1
    return convert_codes((Y >> shift) & mask, (U >> shift) & mask, (V >> shift) & mask, m, oy, wrong.get("oc_used", oc))


# name -> (can it show on a layout?, the keywords of see())
MISTAKES = {
    "a signed load": (lambda s: s["shift"] + s["depth"] == 16, lambda s: dict(signed=True)),
    "the mask dropped": (lambda s: s["shift"] + s["depth"] < 16, lambda s: dict(no_mask=True)),
    "the shift dropped": (lambda s: s["shift"] > 0, lambda s: dict(no_shift=True)),
    "strides taken as elements instead of bytes": (lambda s: True, lambda s: dict(scale=2)),
    "U and V swapped": (lambda s: True, lambda s: dict(swap=True)),
    "sx and sy swapped": (lambda s: s["sx"] != s["sy"], lambda s: dict(swap_shifts=True)),
    "the luma row stride used for chroma": (lambda s: s["y"][2][1] != s["u"][2][1], lambda s: dict(cr=s["y"][2][1])),
    "a 32-bit frame term": (lambda s: True, lambda s: dict(frame32=2 ** 31 + 4098)),
    "oc taken as 128": (lambda s: True, lambda s: dict(oc_used=128.0)),
}
