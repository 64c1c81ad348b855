"""Region tables, pads, geometries and frames of the fused keypoint tests (tests/test_kp_regions.py on the CPU,
tests/test_gpu_keypoint_regions.py on the GPU).  Plain module, no GPU work.

The fused calls (silent_gray_keypoints*, silent_rgb_keypoints[_h]) take ``pad`` and one (rH, rW) region per level.  A region is the
STRIDE of TF1's max_pool(k = the whole level, stride = region, SAME) -- max_value_indices_region of the reference -- and the library
takes one of two paths with it: up to 4 windows per axis on every level run the kernarg cell tables (and, under selection, the sparse
tail), more than that on any axis of any level sends the whole call down the general prefix / suffix path.  ``axis`` below restates
that geometry from the comment of csrc/silent_peaks_plan.h (region_axis) and from oracle/silent_oracle.py (_region_pool_geometry); it
calls neither."""
import math

import numpy as np

from conftest import noise_frame, structured_frame

MAX_WIN, MAX_SEG = 4, 8                 # csrc/silent_peaks.h: kMaxWin, kMaxSeg
E5 = math.e ** .5


def _ceil_div(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- the restatement of region_axis

def axis(size, stride):
    """(windows [(lo, hi)], cuts): out = ceil(size / stride) windows, window j = [j * stride - pad_before, + size) clipped to
    [0, size) with pad_before = ((out - 1) * stride) // 2; the cuts are the distinct window edges (0 and size among them), so the
    axis has len(cuts) - 1 segments."""
    out = _ceil_div(size, stride)
    pad_before = ((out - 1) * stride) // 2
    wins = [(max(j * stride - pad_before, 0), min(j * stride - pad_before + size, size)) for j in range(out)]
    cuts = sorted({0, size} | {e for w in wins for e in w})
    return wins, cuts


def tables(extents, regions):
    """Per level dict(wy, wx: windows per axis; sy, sx: segments per axis; rows, cols: the windows themselves)."""
    out = []
    for (h, w), (rh, rw) in zip(extents, regions):
        (rows, rcut), (cols, ccut) = axis(h, rh), axis(w, rw)
        out.append(dict(wy=len(rows), wx=len(cols), sy=len(rcut) - 1, sx=len(ccut) - 1, rows=rows, cols=cols))
    return out


def path(extents, regions):
    """("cells" | "general", tables): general as soon as one axis of one level has more than MAX_WIN windows or MAX_SEG segments."""
    t = tables(extents, regions)
    general = any(max(l["wy"], l["wx"]) > MAX_WIN or max(l["sy"], l["sx"]) > MAX_SEG for l in t)
    return ("general" if general else "cells"), t


# ----------------------------------------------------------------------------- region families: extents -> one (rH, rW) per level

def _default(ext):
    return [(max(h // 2, 1), max(w // 2, 1)) for h, w in ext]


def _mixed(ext):
    return _default(ext)[:-1] + [(1, 1)]


FAMILIES = {
    "default": _default,                                                        # today's case: 2 or 3 windows
    "one": lambda ext: [(h, w) for h, w in ext],                                # one window per axis
    "over": lambda ext: [(h + 5, w + 9) for h, w in ext],                       # a region larger than the level: still one window
    "four": lambda ext: [(_ceil_div(h, 4), _ceil_div(w, 4)) for h, w in ext],   # 4 windows: the last cell-table case
    "five_cols": lambda ext: [(max(h // 2, 1), _ceil_div(w, 5)) for h, w in ext],   # general because of the columns only
    "five_rows": lambda ext: [(_ceil_div(h, 5), max(w // 2, 1)) for h, w in ext],   # ... of the rows only
    "cells3": lambda ext: [(3, 3) for _ in ext],                                # the reference's centroid_region_shape
    "unit": lambda ext: [(1, 1) for _ in ext],                                  # every pixel its own stride (G3 only)
    "mixed": _mixed,                                                            # general for the whole call because of one level
}
CELLS = ("default", "one", "over", "four")
GENERAL = ("five_cols", "five_rows", "cells3", "mixed")


def regions(family, ext):
    return [(int(rh), int(rw)) for rh, rw in FAMILIES[family](ext)]


# ----------------------------------------------------------------------------- pads

PADS = (0, 1, 2, 3, "big")


def big_pad(ext):
    """The smallest pad that empties the last level (pad_inwards leaves nothing where 2 * pad uses up an axis)."""
    h, w = ext[-1]
    return (min(h, w) + 1) // 2


def pad_of(pad, ext):
    return big_pad(ext) if pad == "big" else int(pad)


# ----------------------------------------------------------------------------- geometries

GEOMETRIES = {
    # the smallest at which every kernel form still has edge and inner tiles (16-row tiles, 56-column waves, 4-wave blocks)
    "G1": dict(mode="gray", hw=(97, 233), geo=dict(scale=2.0, n_levels=4)),
    "G2": dict(mode="gray", hw=(150, 200), geo=dict(center_dimensions=(48, 32), scale=E5)),     # the reference's crops: equal levels
    "G3": dict(mode="gray", hw=(40, 40), geo=dict(scale=2.0, n_levels=2)),                      # "unit" only
    "R1": dict(mode="rgb", hw=(150, 260), geo=dict(scale=2.0, n_levels=4)),
    "R2": dict(mode="rgb", hw=(150, 200), geo=dict(center_dimensions=(48, 32), scale=2.0)),
}


def levels(name):
    """The plan's level table (y0, x0, crop_h, crop_w, zoom_h, zoom_w, out_h, out_w) as LineEndPipeline builds it."""
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    g = GEOMETRIES[name]
    geo = g["geo"]
    if "center_dimensions" in geo:
        return reference_levels(g["hw"], geo["center_dimensions"], geo["scale"])
    return classic_levels(g["hw"], geo["scale"], geo["n_levels"])


def extents(name):
    return [(l[6], l[7]) for l in levels(name)]


# ----------------------------------------------------------------------------- frames

N_FRAMES = 4
_FRAMES = {}


def planted(img, top=255.0):
    """Bright features near the corners and the borders of a structured frame, where the windows of the families differ: a window
    maximum that sits in the middle of a level belongs to every window of every family."""
    h, w, _ = img.shape
    for k, (y, x, ln) in enumerate(((3, 4, 9), (h - 6, w - 14, 9), (4, w - 9, 5), (h - 5, 5, 7), (h // 2, 3, 6), (3, w // 2 + 7, 6),
                                    (h // 3, w - 5, 3), (h - 4, w // 3, 8))):
        img[y, x:x + ln] = top - 4.0 * k
    return img


def frames(hw, channels):
    """[4, H, W, channels] float32, read-only, made once: 0 noise, 1 structured (black background: windows without a positive peak,
    zero plateaus), 2 structured and quantised to multiples of 64 (ties between peaks), 3 = frame 0 with a NaN block, a +inf and a
    -inf pixel (its levels take the dense route)."""
    key = (tuple(hw), channels)
    if key not in _FRAMES:
        h, w = hw
        f0 = noise_frame(7100 + w, h, w, channels)
        f1 = planted(structured_frame(7200 + w, h, w, channels, n_lines=60))
        f2 = planted(structured_frame(7300 + w, h, w, channels, n_lines=40))
        f2 = (np.round(f2 / 64.0) * 64.0).astype(np.float32)
        f3 = f0.copy()
        f3[h // 3:h // 3 + 3, w // 4:w // 4 + 2, 0] = np.nan
        f3[h // 8, w // 9, channels - 1] = np.inf
        f3[(2 * h) // 3, (3 * w) // 4, 0] = -np.inf
        out = np.stack([f0, f1, f2, f3]).astype(np.float32)
        out.setflags(write=False)
        _FRAMES[key] = out
    return _FRAMES[key]
