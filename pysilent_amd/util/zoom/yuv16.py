"""Planar, semi-planar and packed 16-bit YUV surfaces as the (y, u, v) triple of uint16 views the RGB pyramid reads in place
(LineEndPipeline(mode="rgb", rgb_frame_format="yuv420p10" ...), PyramidPlan.run(rgb_frame_format=...))."""

# layout -> rgb_frame_format of the triple.  Planar layouts carry the code in the LOW bits (FFmpeg's yuv4xxp10le / p12le), semi-planar
# and packed ones in the HIGH bits ("...msb"); at depth 16 both coincide.
YUV16_LAYOUTS = {"i010": "yuv420p10", "i210": "yuv422p10", "i410": "yuv444p10", "i012": "yuv420p12", "i212": "yuv422p12", "i412": "yuv444p12",
                 "p010": "yuv420p10msb", "p012": "yuv420p12msb", "p016": "yuv420p16", "p210": "yuv422p10msb", "p216": "yuv422p16",
                 "p410": "yuv444p10msb", "p416": "yuv444p16",
                 "y210": "yuv422p10msb", "y212": "yuv422p12msb", "y216": "yuv422p16"}


def yuv16_planes(surfaces, H, W, layout):
    """(y, u, v) views of 16-bit YUV surfaces ``surfaces`` [n, rows, pitch_elements] (uint16 torch tensor or ndarray; nothing is
    copied), each [n, H, W] or [n, H >> sy, W >> sx] with the layout in its strides -- the triple step() and PyramidPlan.run take for
    the rgb_frame_format YUV16_LAYOUTS[layout].  ``pitch`` counts ELEMENTS.  Luma occupies rows 0 .. H - 1 at ``pitch``:

    * planar "i010" / "i210" / "i410" (and "i012" / "i212" / "i412") -- U then V follow at element offset H * pitch, each row
      ``pitch // 2`` elements ("i410": ``pitch``): H / 2 rows each and rows >= 3 H / 2; H rows and rows >= 2 H; rows >= 3 H;
    * semi-planar "p010" / "p012" / "p016" (H / 2 chroma rows), "p210" / "p216" (H rows), "p410" / "p416" (H rows of W pairs, pitch >=
      2 W) -- interleaved (U, V) element pairs from row H at ``pitch``;
    * packed "y210" / "y212" / "y216" -- Y0 U Y1 V, pitch >= 2 W, rows >= H.

    Bad extents raise ValueError."""
    H, W = int(H), int(W)
    if layout not in YUV16_LAYOUTS:
        raise ValueError("yuv16_planes: layout must be one of %s, got %r" % (", ".join(sorted(YUV16_LAYOUTS)), layout))
    fmt, kind = YUV16_LAYOUTS[layout], {"i": "planar", "p": "semi", "y": "packed"}[layout[0]]
    sx, sy = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[fmt[3:6]]
    if H < 1 or W < 1 or (sy and H % 2) or (sx and W % 2):
        raise ValueError("yuv16_planes: %s needs even %s, got (%d, %d)" % (layout, "H and W" if sy else "W", H, W))
    if getattr(surfaces, "ndim", None) != 3:
        raise ValueError("yuv16_planes: surfaces must be [n, rows, pitch], got shape %s" % (tuple(getattr(surfaces, "shape", ())),))
    if "uint16" not in str(surfaces.dtype):
        raise ValueError("yuv16_planes: surfaces must be uint16, got %s" % (surfaces.dtype,))
    n, rows, pitch = (int(s) for s in surfaces.shape)
    ch, cw = H >> sy, W >> sx
    torch_like = hasattr(surfaces, "as_strided")
    if torch_like:                                     # torch: strides in elements
        sn, sr, sp = (int(s) for s in surfaces.stride())
    else:                                              # NumPy: strides in bytes
        if any(int(s) % 2 for s in surfaces.strides):
            raise ValueError("yuv16_planes: the byte strides of uint16 surfaces must be even, got %s" % (tuple(surfaces.strides),))
        sn, sr, sp = (int(s) // 2 for s in surfaces.strides)
    if sp != 1 and pitch > 1:
        raise ValueError("yuv16_planes: the elements of a surface row must be adjacent (stride %d)" % sp)

    def view(offset, shape, strides):
        """elements [offset + f * sn + r * strides[0] + c * strides[1]] of the surfaces' storage"""
        if torch_like:                                 # a view, never a copy
            return surfaces.as_strided((n,) + shape, (sn,) + strides, surfaces.storage_offset() + offset)
        import numpy as np
        if not surfaces.flags.c_contiguous:
            raise ValueError("yuv16_planes: NumPy surfaces must be C-contiguous")
        return np.lib.stride_tricks.as_strided(surfaces.reshape(-1)[offset:], (n,) + shape, tuple(2 * s for s in (sn,) + strides),
                                               writeable=surfaces.flags.writeable)

    def need(ok, what):
        if not ok:
            raise ValueError("yuv16_planes: surfaces [%d, %d, %d] do not hold %d x %d %s (%s)" % (n, rows, pitch, H, W, layout, what))

    if kind == "packed":
        need(rows >= H and pitch >= 2 * W, "rows >= H, pitch >= 2 W")
        return (view(0, (H, W), (sr, 2)), view(1, (H, cw), (sr, 4)), view(3, (H, cw), (sr, 4)))
    need(pitch >= W, "pitch >= W")
    y = view(0, (H, W), (sr, 1))
    if kind == "semi":
        need(rows >= H + ch and pitch >= 2 * cw, "rows >= H + chroma rows, pitch >= the elements of a chroma row")
        return (y, view(H * sr, (ch, cw), (sr, 2)), view(H * sr + 1, (ch, cw), (sr, 2)))
    # planar: the chroma planes are packed behind the luma rows at their own pitch, so the surface rows must be adjacent
    cp = pitch if sx == 0 else pitch // 2
    need(sr == pitch, "planar layouts need adjacent surface rows")
    need(cp >= cw and rows * pitch >= H * pitch + 2 * ch * cp, "rows >= %s" % {"420": "3 H / 2", "422": "2 H", "444": "3 H"}[fmt[3:6]])
    return (y, view(H * pitch, (ch, cw), (cp, 1)), view(H * pitch + ch * cp, (ch, cw), (cp, 1)))
