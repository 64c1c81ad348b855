"""Level geometry for silent_pyramid_plan_create that classic_levels() and reference_levels() never produce (test
infrastructure, like tests/chain_weights.py).

Every plan the project ran before this file came from those two generators, and they keep fixed what the planner and its kernels
depend on: a same-crop plan is always the whole frame (origin 0, the crop edge IS the frame edge), the unit level is always level
0 and the only one, zoom is isotropic and descending, never upsamples, classic canvases equal their zoom, the reference's crops are
centred and nested with the outermost last, and no axis is degenerate.  A kernel that ignores the crop origin, swaps y0 and x0,
mirrors at the frame edge, applies one axis' ratio to both, writes levels in sorted order or puts a second unit level at the
first one's offset returns the same pyramid on them.  CASES below vary each of those properties on its own, on frames of about
150 x 316 (W % 4 == 0: the walk's 16-byte loader and its alignment shift) and 149 x 317 (single-float loader): every crop wider
than 144 crosses two walk strips, and every unit level two 60-column unit tiles and two tile rows.

A level is the tuple (src_y0, src_x0, src_h, src_w, zoom_h, zoom_w, out_h, out_w) of silent_pyr_level."""
import math

import numpy as np

E = math.e ** .5
FA, FB = (150, 316), (149, 317)
MIRROR_NEAR_MIN = 5            # kMirrorNearMin (csrc/silent_common.h): the shortest axis of a unit level
MAX_LEVELS = 16                # SILENT_MAX_LEVELS


def is_unit(lv):
    """The planner's classification: zoom factor exactly 1 on both axes, and both long enough for the one-reflection mirror."""
    return lv[4] == lv[2] and lv[5] == lv[3] and lv[2] >= MIRROR_NEAR_MIN and lv[3] >= MIRROR_NEAR_MIN


def ladder(crop, ratio, n_gen, unit_pad=(0, 0), gen_pad=None, order=None):
    """One unit level + n_gen general levels on one crop at ratio ** -k.  unit_pad: canvas of the unit level beyond its crop;
    gen_pad[k]: canvas of general level k relative to its zoom (+: zero fill, -: the copy clips); order: a permutation of
    0 .. n_gen (0 = the unit level)."""
    y0, x0, ch, cw = crop
    lv = [(y0, x0, ch, cw, ch, cw, ch + unit_pad[0], cw + unit_pad[1])]
    for k in range(1, n_gen + 1):
        zh, zw = max(int(round(ch / ratio ** k)), 1), max(int(round(cw / ratio ** k)), 1)
        ph, pw = gen_pad[k - 1] if gen_pad else (0, 0)
        lv.append((y0, x0, ch, cw, zh, zw, max(zh + ph, 1), max(zw + pw, 1)))
    return [lv[i] for i in order] if order else lv


def _lv(y0, x0, ch, cw, zh, zw, oh=None, ow=None):
    return (y0, x0, ch, cw, zh, zw, zh if oh is None else oh, zw if ow is None else ow)


# The three sub-windows of both frames: touching no frame edge, flush with the top-left, flush with the bottom-right; between them
# and the two frames src_x0 % 4 takes all four residues (the walk's wp3.shift = (src_x0 * 3) % 4 on the 316-wide frame)
SUB = {
    "in": {FA: (23, 41, 101, 233), FB: (14, 42, 112, 251)},            # x0 % 4 = 1, 2
    "tl": {FA: (0, 0, 120, 250), FB: (0, 0, 99, 230)},                 # 0
    "br": {FA: (53, 115, 97, 201), FB: (38, 66, 111, 251)},            # 3, 2
    "in3": {FA: (19, 7, 118, 290), FB: (9, 3, 130, 301)},              # 3
}
PADS = [(3, -4), (-2, 5), (-3, -6)]          # general canvases larger and smaller than their zoom, per axis

CASES = {}


def _case(name, frame, levels, *classes):
    assert name not in CASES
    CASES[name] = dict(frame=frame, levels=[tuple(int(v) for v in l) for l in levels], classes=frozenset(classes))


# ---- sub-window ladders (one unit level + 2 - 3 general levels on the same crop, ratios 2, e^.5, 1.5)
for _pos, _frame, _ratio, _n in (("in", FA, 2.0, 3), ("tl", FA, E, 3), ("br", FA, 1.5, 3), ("in", FB, E, 2), ("br", FB, 2.0, 3),
                                 ("in3", FA, 1.5, 2), ("tl", FB, 1.5, 3)):
    _case("sub_%s_%d_%.2f" % (_pos, _frame[1], _ratio), _frame, ladder(SUB[_pos][_frame], _ratio, _n), "sub_window",
          *(("crop_edge",) if _pos != "tl" else ()))
for _pos, _frame, _ratio in (("in", FA, E), ("tl", FA, 2.0), ("br", FA, 1.5), ("in3", FB, 2.0)):
    _case("ucanvas_%s_%d" % (_pos, _frame[1]), _frame, ladder(SUB[_pos][_frame], _ratio, 3, unit_pad=(5, 7)), "sub_window", "unit_canvas",
          *(("crop_edge",) if _pos != "tl" else ()))
for _pos, _frame, _ratio in (("in", FA, 1.5), ("tl", FB, E), ("br", FA, 2.0), ("br", FB, 1.5)):
    _case("gcanvas_%s_%d" % (_pos, _frame[1]), _frame, ladder(SUB[_pos][_frame], _ratio, 3, gen_pad=PADS), "sub_window", "canvas_clip",
          *(("crop_edge",) if _pos != "tl" else ()))
for _pos, _frame, _ratio, _order in (("in", FA, 2.0, [2, 3, 1, 0]), ("tl", FA, 1.5, [1, 3, 2, 0]), ("br", FB, E, [2, 3, 1, 0]),
                                     ("in3", FA, E, [3, 1, 2, 0])):
    _case("ulast_%s_%d" % (_pos, _frame[1]), _frame, ladder(SUB[_pos][_frame], _ratio, 3, order=_order), "sub_window", "order",
          *(("crop_edge",) if _pos != "tl" else ()))
# (a ratio below e^.5 keeps five output rows of the first level in flight: the stream kernels' dense slot layout)
_case("dense_in_317", FB, ladder(SUB["in"][FB], 2 ** .5, 3), "sub_window", "crop_edge")
_case("dense_br_316", FA, ladder(SUB["br"][FA], 2 ** .5, 3, unit_pad=(5, 7), gen_pad=PADS), "sub_window", "crop_edge", "unit_canvas", "canvas_clip")

# ---- anisotropic zoom, and a level that is unit along one axis only
_c = SUB["in"][FA]
_case("aniso_316", FA, [_c + (101, 233, 101, 233), _lv(*_c, 50, 77), _lv(*_c, 33, 116), _lv(*_c, 13, 58)], "sub_window", "crop_edge", "aniso")
_c = SUB["br"][FB]
_case("aniso_317", FB, [_lv(*_c, 37, 125), _c + (111, 251, 111, 251), _lv(*_c, 55, 63)], "sub_window", "crop_edge", "aniso", "order")
_c = SUB["in3"][FA]
_case("unit_one_axis_316", FA, [_c + (118, 290, 118, 290), _lv(*_c, 118, 145), _lv(*_c, 59, 290)], "sub_window", "crop_edge", "aniso")
_case("unit_one_axis_317", FB, [_lv(14, 42, 112, 251, 112, 100), _lv(14, 42, 112, 251, 40, 251)], "crop_edge", "aniso")

# ---- unit-level counts
_case("two_units_316", FA, [_lv(3, 9, 70, 150, 70, 150), _lv(3, 9, 70, 150, 35, 75), _lv(60, 130, 90, 186, 90, 186),
                            _lv(60, 130, 90, 186, 45, 93)], "crop_edge", "two_units")
_case("two_units_317", FB, [_lv(40, 100, 80, 170, 40, 85), _lv(40, 100, 80, 170, 80, 170, 83, 175), _lv(0, 0, 149, 317, 75, 159),
                            _lv(10, 21, 66, 131, 66, 131)], "crop_edge", "two_units", "order", "unit_canvas")
_case("units_only_316", FA, [_lv(5, 6, 30, 200, 30, 200), _lv(100, 99, 50, 70, 50, 70, 52, 70), _lv(0, 0, 150, 316, 150, 316)],
      "crop_edge", "two_units")
_case("no_unit_316", FA, ladder(SUB["in"][FA], 2.0, 3)[1:], "crop_edge", "no_unit")
_case("no_unit_317", FB, ladder(SUB["br"][FB], E, 3, gen_pad=PADS)[1:], "crop_edge", "no_unit", "canvas_clip")

# ---- upsampled levels (step < 1)
_case("up_1.5_316", FA, [_lv(30, 50, 60, 110, 60, 110), _lv(30, 50, 60, 110, 90, 165), _lv(30, 50, 60, 110, 30, 55)], "crop_edge", "upsample")
_case("up_2_one_axis_317", FB, [_lv(20, 33, 50, 180, 100, 180), _lv(20, 33, 50, 180, 25, 90), _lv(70, 5, 70, 60, 70, 120)],
      "crop_edge", "upsample", "aniso")

# ---- degenerate axes
_case("zoom_h_1_316", FA, [_lv(50, 60, 40, 200, 1, 100), _lv(50, 60, 40, 200, 20, 100), _lv(7, 300, 100, 9, 50, 1)], "crop_edge", "degenerate")
_case("row_crop_317", FB, [_lv(70, 10, 1, 200, 1, 100), _lv(70, 10, 1, 200, 1, 200), _lv(3, 311, 120, 1, 60, 1)], "crop_edge", "degenerate")
_case("four_rows_316", FA, [_lv(140, 100, 4, 200, 4, 200), _lv(140, 100, 4, 200, 2, 100), _lv(20, 310, 100, 4, 100, 4)], "crop_edge", "degenerate")
_case("narrow_rgb_317", FB, [_lv(10, 10, 50, 6, 50, 6), _lv(10, 10, 50, 6, 25, 3), _lv(40, 300, 80, 7, 40, 4)], "crop_edge", "degenerate")

# ---- crop layouts
# off-centre and nested: the inner crops share the top-left / the bottom-right corner with the outer one, which is not last
_case("nested_316", FA, [_lv(20, 30, 60, 120, 30, 60), _lv(20, 30, 120, 250, 30, 62), _lv(80, 160, 60, 120, 40, 80)], "crop_edge", "nested", "order")
_case("nested_317", FB, [_lv(9, 13, 140, 300, 140, 300), _lv(9, 13, 70, 150, 35, 75), _lv(9, 13, 140, 300, 35, 75, 35, 80),
                         _lv(79, 163, 70, 150, 47, 100), _lv(9, 163, 70, 150, 24, 50)], "crop_edge", "nested", "order")
_case("overlap_316", FA, [_lv(0, 0, 100, 200, 50, 100), _lv(50, 116, 100, 200, 50, 100), _lv(30, 57, 90, 203, 30, 68)], "crop_edge", "layout")
_case("disjoint_317", FB, [_lv(0, 0, 70, 150, 35, 75), _lv(79, 167, 70, 150, 35, 75), _lv(0, 160, 70, 157, 47, 105)], "crop_edge", "layout")
_case("nine_crops_316", FA, [_lv(3 * k, 5 * k + 1, 60 + 8 * k, 150 + 14 * k, 30 + k, 75 - 3 * k) for k in range(9)], "crop_edge", "layout")

# ---- the trimmed walk: general levels only, a sliver of at most px / 2 behind the last strip
_case("trim_300_316", FA, [_lv(11, 13, 120, 300, 60, 150), _lv(11, 13, 120, 300, 30, 75), _lv(11, 13, 120, 300, 15, 38)], "crop_edge", "no_unit", "trim")
_case("trim_266_317", FB, ladder((2, 18, 140, 266), E, 3)[1:], "crop_edge", "no_unit", "trim")
_case("trim_nested_316", FA, [_lv(40, 100, 60, 150, 30, 75), _lv(11, 13, 120, 300, 60, 150), _lv(11, 13, 120, 300, 30, 75)],
      "crop_edge", "no_unit", "nested")

# ---- scipy's dead last row (48 -> 24) and dead last column (90 -> 45) inside sub-crops
_case("dead_316", FA, [_lv(31, 57, 48, 200, 48, 200), _lv(31, 57, 48, 200, 24, 100), _lv(60, 201, 80, 90, 40, 45, 42, 47)], "crop_edge", "dead")
_case("dead_317", FB, [_lv(100, 226, 48, 90, 24, 45), _lv(100, 226, 48, 90, 48, 90), _lv(0, 0, 48, 317, 24, 159)], "crop_edge", "dead", "order")


# ----------------------------------------------------------------------------- validity, random draws

def is_valid(frame_hw, levels):
    """The validity rules of silent_pyramid_plan_create, nothing else."""
    H, W = frame_hw
    if not (1 <= len(levels) <= MAX_LEVELS):
        return False
    for y0, x0, ch, cw, zh, zw, oh, ow in levels:
        if not (ch >= 1 and cw >= 1 and y0 >= 0 and x0 >= 0 and y0 + ch <= H and x0 + cw <= W and min(zh, zw, oh, ow) >= 1):
            return False
    return True


def random_levels(rng, frame_hw, channels=1):
    """A seeded draw of valid generic levels that mixes the properties of CASES: crops anywhere (flush with an edge one time in
    three), shared or not, unit levels anywhere and any number, anisotropic zoom, upsampling, canvases around their zoom,
    degenerate axes, any order.  ``channels`` only biases the widths (an RGB walk wants a crop of 8 columns or more)."""
    H, W = frame_hw

    def crop():
        ch = int(rng.integers(1, H + 1)) if rng.random() < 0.15 else int(rng.integers(max(H // 3, 1), H + 1))
        cw = int(rng.integers(1, W + 1)) if rng.random() < 0.15 else int(rng.integers(max(W // 3, 1), W + 1))
        if channels == 3 and rng.random() < 0.8:
            cw = min(max(cw, 8), W)
        edge = rng.integers(0, 6)
        y0 = 0 if edge == 0 else H - ch if edge == 1 else int(rng.integers(0, H - ch + 1))
        x0 = 0 if edge == 0 else W - cw if edge == 1 else int(rng.integers(0, W - cw + 1))
        return y0, x0, ch, cw

    def zoomed(n):
        kind = rng.integers(0, 10)
        if kind == 0:
            return n                                          # unit along this axis
        if kind == 1:
            return max(int(round(n * rng.uniform(1.0, 2.2))), 1)        # upsampled
        if kind == 2:
            return int(rng.integers(1, 4))
        return max(int(round(n / float(rng.choice([1.2, 2 ** .5, 1.5, E, 2.0, 2.7, 4.0])) ** int(rng.integers(1, 3)))), 1)

    n = int(rng.integers(1, 8))
    shared = crop() if rng.random() < 0.6 else None
    levels = []
    for _ in range(n):
        y0, x0, ch, cw = shared if shared is not None and rng.random() < 0.8 else crop()
        if rng.random() < 0.25:
            zh, zw = ch, cw
        elif rng.random() < 0.6:
            r = float(rng.choice([1.5, E, 2.0])) ** int(rng.integers(1, 4))
            zh, zw = max(int(round(ch / r)), 1), max(int(round(cw / r)), 1)
        else:
            zh, zw = zoomed(ch), zoomed(cw)
        oh, ow = zh, zw
        if rng.random() < 0.4:
            oh, ow = max(zh + int(rng.integers(-6, 8)), 1), max(zw + int(rng.integers(-6, 8)), 1)
        levels.append((y0, x0, ch, cw, zh, zw, oh, ow))
    assert is_valid(frame_hw, levels)
    return levels


RANDOM_SEEDS = tuple(range(40))


def random_case(seed):
    """(frame_hw, channels, levels) of seed ``seed``: what tests/test_gpu_plan_geometry.py and the CPU attainability test run."""
    rng = np.random.default_rng([int(seed), 20240])
    frame_hw = (int(rng.integers(20, 160)), int(rng.integers(20, 330)))
    channels = 1 if seed % 2 == 0 else 3
    if channels == 3 and rng.random() < 0.5:
        frame_hw = (frame_hw[0], max(frame_hw[1] // 4 * 4, 8))
    return frame_hw, channels, random_levels(rng, frame_hw, channels)


def frames_of(frame_hw, channels, n=3, seed=0):
    """Distinct noise frames (conftest.noise_frame)."""
    from conftest import noise_frame
    return np.stack([noise_frame(4100 + 7 * seed + i, frame_hw[0], frame_hw[1], channels) for i in range(n)])


def poisoned_inside(frame, levels):
    """A NaN on the last row / column of every crop (under a dead row or column where a level has one), an inf on its first
    pixel, a NaN near its middle."""
    f = np.array(frame, np.float32)
    c = f.shape[2]
    for k, (y0, x0, ch, cw) in enumerate(sorted({l[:4] for l in levels})):
        f[y0 + ch - 1, x0 + cw - 1, k % c] = np.nan
        f[y0, x0, (k + 1) % c] = np.inf
        f[y0 + ch // 2, x0 + (2 * cw) // 3, (k + 2) % c] = np.nan
    return f


# ----------------------------------------------------------------------------- references

def extents(levels):
    return [(l[6], l[7]) for l in levels]


def split(flat, levels, channels):
    """A packed pyramid of one frame -> its levels [oh, ow, C], in the given order."""
    out, off = [], 0
    for oh, ow in extents(levels):
        out.append(np.asarray(flat[off:off + oh * ow * channels]).reshape(oh, ow, channels))
        off += oh * ow * channels
    assert off == len(flat)
    return out


def oracle_pyramid(frame, levels):
    """Per-level reference through the C oracle's so_zoom_level (float64 tap products and sum, one rounding)."""
    import c_oracle as co
    frame = np.ascontiguousarray(frame, np.float32)
    return [co.zoom_level(frame, *lv) for lv in levels]


def python_pyramid(frame, levels):
    """The same through silent_oracle.spline5_zoom on the crop and a clipped copy into a zero canvas."""
    import silent_oracle as so
    out = []
    for y0, x0, ch, cw, zh, zw, oh, ow in levels:
        canvas = np.zeros((oh, ow, frame.shape[2]), np.float32)
        ym, xm = min(zh, oh), min(zw, ow)
        for c in range(frame.shape[2]):
            canvas[:ym, :xm, c] = so.spline5_zoom(np.ascontiguousarray(frame[y0:y0 + ch, x0:x0 + cw, c]), zh, zw)[:ym, :xm]
        out.append(canvas)
    return out


def scipy_applies(lv):
    """scipy.ndimage.zoom takes ONE factor per axis and rounds the extent itself: usable where it lands on the level's zoom."""
    _, _, ch, cw, zh, zw, _, _ = lv
    return int(round(ch * (zh / ch))) == zh and int(round(cw * (zw / cw))) == zw


def scipy_level(frame, lv):
    from scipy import ndimage
    y0, x0, ch, cw, zh, zw, oh, ow = lv
    canvas = np.zeros((oh, ow, frame.shape[2]), np.float32)
    ym, xm = min(zh, oh), min(zw, ow)
    for c in range(frame.shape[2]):
        z = ndimage.zoom(np.ascontiguousarray(frame[y0:y0 + ch, x0:x0 + cw, c]), (zh / ch, zw / cw), order=5, prefilter=False)
        assert z.shape == (zh, zw)
        canvas[:ym, :xm, c] = z[:ym, :xm]
    return canvas


def dead_axes(lv):
    """(last output row is dead, last output column is dead): scipy's mode-'constant' artefact, silent_oracle.zoom_axis_table."""
    import silent_oracle as so
    return tuple(bool(n_out > 1 and not so.zoom_axis_table(n_in, n_out)[2][-1].any()) for n_in, n_out in ((lv[2], lv[4]), (lv[3], lv[5])))


def zero_mask(lv):
    """[oh, ow] bool: the canvas pixels that are exactly 0 whatever the frame holds -- beyond the zoomed crop, and dead rows / columns."""
    _, _, _, _, zh, zw, oh, ow = lv
    dr, dc = dead_axes(lv)
    m = np.ones((oh, ow), bool)
    m[:min(zh - int(dr), oh), :min(zw - int(dc), ow)] = False
    return m


def _taps(n_in, n_out, origin=0, frame_n=None, keep_dead=False):
    """Indices into the FRAME axis and float64 weights.  frame_n: mirror at the frame edge (the taps run on past the crop) instead
    of at the crop edge.  keep_dead: weights also for a coordinate that rounds to just above n_in - 1."""
    import silent_oracle as so
    base, idx, w = so.zoom_axis_table(n_in, n_out)
    idx = idx + origin
    if frame_n is not None:
        idx = np.array([[so.mirror_index(int(b) - 2 + j + origin, frame_n) for j in range(6)] for b in base])
    if keep_dead:
        step = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
        w = np.array([so._spline5_weights(o * step - int(base[o])) for o in range(n_out)])
    return idx, w


def evaluate(frame, levels, origin="given", mirror="crop", swap_zoom=False, clip=True, order="given", second_unit="own", dead="zero",
             dtype=np.float64):
    """The pyramid of one frame as a flat packed buffer, with the named mistakes switched on one at a time (MUTANTS).  With the
    defaults it is the oracle's definition (test_plan_geometry.py asserts that, bit for bit)."""
    H, W, C = frame.shape
    f = frame.astype(dtype)
    ext = extents(levels)
    offs = np.concatenate([[0], np.cumsum([oh * ow * C for oh, ow in ext])]).astype(np.int64)
    flat = np.zeros(int(offs[-1]), np.float32)
    slots = list(range(len(levels)))
    if order == "sorted":            # finest first, as the walk sorts its levels: level k of the sorted list lands in slot k
        slots = sorted(slots, key=lambda l: -(levels[l][5] / levels[l][3]))
    units = [l for l in range(len(levels)) if is_unit(levels[l])]
    for slot, l in enumerate(slots):
        y0, x0, ch, cw, zh, zw, oh, ow = levels[l]
        if origin == "ignored":
            y0 = x0 = 0
        elif origin == "swapped":
            y0, x0 = min(x0, H - ch), min(y0, W - cw)
        if swap_zoom:
            zh, zw = zw, zh
        iy, wy = _taps(ch, zh, y0, H if mirror == "frame" else None, dead == "kept")
        ix, wx = _taps(cw, zw, x0, W if mirror == "frame" else None, dead == "kept")
        acc = np.zeros((zh, zw, C), dtype)
        for a in range(6):
            rows = f[iy[:, a]]
            for b in range(6):
                acc += (wy[:, a].astype(dtype)[:, None] * wx[:, b].astype(dtype)[None, :])[:, :, None] * rows[:, ix[:, b]]
        z = acc.astype(np.float32)
        at = int(offs[slot])
        if second_unit == "first" and len(units) >= 2 and l == units[1]:
            at = int(offs[units[0]])
        room = len(flat) - at
        if clip:
            canvas = np.zeros((oh, ow, C), np.float32)
            canvas[:min(zh, oh), :min(zw, ow)] = z[:min(zh, oh), :min(zw, ow)]
            n = min(canvas.size, room)
            flat[at:at + n] = canvas.reshape(-1)[:n]
        else:                        # every zoomed column of the first min(zoom_h, out_h) rows at the canvas' row stride
            for oy in range(min(zh, oh)):
                p = at + oy * ow * C
                n = max(min(zw * C, len(flat) - p), 0)
                flat[p:p + n] = z[oy].reshape(-1)[:n]
    return flat


# name -> (keyword of evaluate(), the case classes meant to catch it)
MUTANTS = {
    "origin_ignored": (dict(origin="ignored"), ("crop_edge",)),
    "origin_swapped": (dict(origin="swapped"), ("crop_edge",)),
    "frame_edge_mirror": (dict(mirror="frame"), ("crop_edge",)),
    "zoom_swapped": (dict(swap_zoom=True), ("aniso",)),
    "canvas_not_clipped": (dict(clip=False), ("canvas_clip",)),
    "sorted_order": (dict(order="sorted"), ("order",)),
    "second_unit_at_first": (dict(second_unit="first"), ("two_units",)),
    "dead_row_kept": (dict(dead="kept"), ("dead",)),
}


def float32_pyramid(frame, levels):
    """torch float32: the 36-tap sums as two separable passes with float32 weights -- a float32 evaluation in another order than
    the oracle's (and than a fused 36-product sum)."""
    import torch
    import silent_oracle as so
    t = torch.from_numpy(np.ascontiguousarray(frame, np.float32))
    out = []
    for y0, x0, ch, cw, zh, zw, oh, ow in levels:
        _, iy, wy = so.zoom_axis_table(ch, zh)
        _, ix, wx = so.zoom_axis_table(cw, zw)
        crop = t[y0:y0 + ch, x0:x0 + cw]
        wy32, wx32 = torch.from_numpy(wy.astype(np.float32)), torch.from_numpy(wx.astype(np.float32))
        v = torch.zeros((zh, cw, t.shape[2]), dtype=torch.float32)
        for a in range(6):
            v = v + wy32[:, a, None, None] * crop[torch.from_numpy(iy[:, a])]
        h = torch.zeros((zh, zw, t.shape[2]), dtype=torch.float32)
        for b in range(6):
            h = h + wx32[None, :, b, None] * v[:, torch.from_numpy(ix[:, b])]
        canvas = np.zeros((oh, ow, frame.shape[2]), np.float32)
        canvas[:min(zh, oh), :min(zw, ow)] = h.numpy()[:min(zh, oh), :min(zw, ow)]
        out.append(canvas)
    return out


def assert_levels_close(got_levels, want_levels, tag):
    """THE assertion of tests/test_gpu_plan_geometry.py: the project's range-relative 1e-5 and the element-wise rounding bound."""
    import err_bound as eb
    from conftest import assert_close
    assert len(got_levels) == len(want_levels)
    for got, want in zip(got_levels, want_levels):
        assert_close(got, want, 1e-5, scale=255.0, what=tag, bound=eb.zoom(want))


# ----------------------------------------------------------------------------- routes

def _stream_slots(layout, g):
    return (4, 3, 2, 2, 1, 1, 1)[g] if layout == 0 else (5, 4, 3, 2, 2, 1, 1)[g]


def stream_layout(levels):
    """Which slot layout of the stream kernels' row programs a single-channel plan gets (0, 1), or None where it is not streamable:
    the planner's own test restated -- one unit level with a canvas no smaller than its crop, 1 - 7 general levels on that crop,
    no two output rows of a level alive in one slot, none completing together, at most 64 outputs per 56-column wave whose taps stay
    inside its 64 lanes.  test_plan_geometry.py checks it against plan.streamable on every case."""
    import silent_oracle as so
    TH, ROWS, COLS = 16, 24, 56
    units = [l for l in levels if is_unit(l)]
    gens = [l for l in levels if not is_unit(l)]
    if len(units) != 1 or not 1 <= len(gens) <= 7:
        return None
    u = units[0]
    if u[6] < u[2] or u[7] < u[3] or any(g[:4] != u[:4] for g in gens):
        return None
    tiles_y = (u[6] + TH - 1) // TH
    waves_x = (u[7] + 4 * COLS - 1) // (4 * COLS) * 4
    for layout in (0, 1):
        ok = True
        for g, lv in enumerate(gens):
            dr, dc = dead_axes(lv)
            zr, zc = min(lv[4] - int(dr), lv[6]), min(lv[5] - int(dc), lv[7])
            yb, xb = so.zoom_axis_table(lv[2], lv[4])[0], so.zoom_axis_table(lv[3], lv[5])[0]
            used, done = set(), set()
            for oy in range(zr):
                t = int(yb[oy]) // TH
                if t >= tiles_y:
                    ok = False
                slot = oy % _stream_slots(layout, g)
                for j in range(6):
                    i = int(yb[oy]) - t * TH + 2 + j
                    if not 0 <= i < ROWS or (t, i, slot) in used or (j == 5 and (t, i) in done):
                        ok = False
                    used.add((t, i, slot))
                    if j == 5:
                        done.add((t, i))
            for wx in range(waves_x):
                cols = [int(x) - wx * COLS + 2 for x in xb[:zc] if wx * COLS <= x < (wx + 1) * COLS]
                if len(cols) > 64 or any(c < 0 or c + 5 > 63 for c in cols):
                    ok = False
        if ok:
            return layout
    return None


def route_tags(levels, channels, streamable, walk_plans):
    """The routes a plan takes, from what the library reports (plan.streamable, plan.walk_plans) and the geometry."""
    units = [l for l in levels if is_unit(l)]
    gens = [l for l in levels if not is_unit(l)]
    tags = set()
    if channels == 1:
        if streamable:
            tags.add("stream%d" % stream_layout(levels))
        else:
            tags.add("unit_region")
            if len(units) >= 2:
                tags.add("multi_unit_fused")
        return tags
    n_plans, px = walk_plans
    if n_plans == 0:
        return {"unit_region"}
    same_crop = len(units) == 1 and gens and all(g[:4] == units[0][:4] for g in gens)
    if same_crop and n_plans == 1:
        return {"walk_single"}
    if len(gens) >= 2 and n_plans == len(units) + 1:
        outer = next(o for o in gens if all(d[0] >= o[0] and d[1] >= o[1] and d[0] + d[2] <= o[0] + o[2] and d[1] + d[3] <= o[1] + o[3]
                                            for d in gens))
        tags.add("walk_union_borders" if any(g[:4] != outer[:4] for g in gens) else "walk_union")
        strip = 4 * px
        if outer[3] > strip and 0 < outer[3] % strip <= px // 2:
            tags.add("walk_trimmed")
    elif n_plans == len(levels):
        tags.add("walk_per_level")
    return tags


REQUIRED_ROUTES = ("stream0", "stream1", "walk_single", "walk_union_borders", "walk_per_level", "walk_trimmed", "unit_region",
                   "multi_unit_fused")

# name -> ((streamable, walk_plans) of the 1-channel plan, the same of the 3-channel plan), as silent_pyramid_plan_create decides
# them on the host (recorded with the host-only build; tests/test_plan_geometry.py asserts them and the routes they stand for)
ROUTES = {
    "sub_in_316_2.00":     ((True, (0, 0)), (False, (1, 36))),
    "sub_tl_316_1.65":     ((True, (0, 0)), (False, (1, 32))),
    "sub_br_316_1.50":     ((True, (0, 0)), (False, (1, 28))),
    "sub_in_317_1.65":     ((True, (0, 0)), (False, (1, 32))),
    "sub_br_317_2.00":     ((True, (0, 0)), (False, (1, 36))),
    "sub_in3_316_1.50":    ((True, (0, 0)), (False, (1, 28))),
    "sub_tl_317_1.50":     ((True, (0, 0)), (False, (1, 28))),
    "ucanvas_in_316":      ((True, (0, 0)), (False, (1, 32))),
    "ucanvas_tl_316":      ((True, (0, 0)), (False, (1, 36))),
    "ucanvas_br_316":      ((True, (0, 0)), (False, (1, 28))),
    "ucanvas_in3_317":     ((True, (0, 0)), (False, (1, 36))),
    "gcanvas_in_316":      ((True, (0, 0)), (False, (1, 28))),
    "gcanvas_tl_317":      ((True, (0, 0)), (False, (1, 32))),
    "gcanvas_br_316":      ((True, (0, 0)), (False, (1, 36))),
    "gcanvas_br_317":      ((True, (0, 0)), (False, (1, 28))),
    "ulast_in_316":        ((True, (0, 0)), (False, (1, 36))),
    "ulast_tl_316":        ((True, (0, 0)), (False, (1, 28))),
    "ulast_br_317":        ((False, (0, 0)), (False, (1, 32))),
    "ulast_in3_316":       ((True, (0, 0)), (False, (1, 32))),
    "dense_in_317":        ((True, (0, 0)), (False, (1, 28))),
    "dense_br_316":        ((True, (0, 0)), (False, (1, 28))),
    "aniso_316":           ((True, (0, 0)), (False, (1, 32))),
    "aniso_317":           ((True, (0, 0)), (False, (1, 36))),
    "unit_one_axis_316":   ((False, (0, 0)), (False, (0, 0))),
    "unit_one_axis_317":   ((False, (0, 0)), (False, (0, 0))),
    "two_units_316":       ((False, (0, 0)), (False, (4, 36))),
    "two_units_317":       ((False, (0, 0)), (False, (3, 28))),
    "units_only_316":      ((False, (0, 0)), (False, (3, 36))),
    "no_unit_316":         ((False, (0, 0)), (False, (1, 36))),
    "no_unit_317":         ((False, (0, 0)), (False, (1, 32))),
    "up_1.5_316":          ((False, (0, 0)), (False, (0, 0))),
    "up_2_one_axis_317":   ((False, (0, 0)), (False, (0, 0))),
    "zoom_h_1_316":        ((False, (0, 0)), (False, (3, 36))),
    "row_crop_317":        ((False, (0, 0)), (False, (0, 0))),
    "four_rows_316":       ((False, (0, 0)), (False, (0, 0))),
    "narrow_rgb_317":      ((False, (0, 0)), (False, (0, 0))),
    "nested_316":          ((False, (0, 0)), (False, (1, 28))),
    "nested_317":          ((False, (0, 0)), (False, (2, 28))),
    "overlap_316":         ((False, (0, 0)), (False, (3, 36))),
    "disjoint_317":        ((False, (0, 0)), (False, (3, 28))),
    "nine_crops_316":      ((False, (0, 0)), (False, (0, 0))),
    "trim_300_316":        ((False, (0, 0)), (False, (1, 36))),
    "trim_266_317":        ((False, (0, 0)), (False, (1, 32))),
    "trim_nested_316":     ((False, (0, 0)), (False, (1, 28))),
    "dead_316":            ((False, (0, 0)), (False, (3, 36))),
    "dead_317":            ((False, (0, 0)), (False, (3, 36))),
}
