"""Planar, semi-planar and packed 8-bit YUV surfaces as the (y, u, v) triple of views the RGB pyramid reads in place
(LineEndPipeline(mode="rgb", rgb_frame_format="yuv420" / "yuv422" / "yuv444"), PyramidPlan.run(rgb_frame_format=...))."""

# layout -> (rgb_frame_format of the triple, kind)
YUV_LAYOUTS = {"i420": ("yuv420", "planar"), "yv12": ("yuv420", "planar"), "i422": ("yuv422", "planar"), "i444": ("yuv444", "planar"),
               "nv12": ("yuv420", "semi"), "nv21": ("yuv420", "semi"), "nv16": ("yuv422", "semi"),
               "yuyv": ("yuv422", "packed"), "uyvy": ("yuv422", "packed")}


def yuv_planes(surfaces, H, W, layout):
    """(y, u, v) views of 8-bit YUV surfaces ``surfaces`` [n, rows, pitch] (uint8 torch tensor or ndarray; nothing is copied), each
    [n, H, W] or [n, H >> sy, W >> sx] with the layout in its strides -- the triple step() and PyramidPlan.run take for the
    rgb_frame_format YUV_LAYOUTS[layout][0].  Luma occupies rows 0 .. H - 1 at ``pitch``:

    * planar -- the two chroma planes follow at byte offset H * pitch, each row ``pitch // 2`` bytes ("i444": ``pitch``):
      "i420" / "yv12": U then V (V then U), H / 2 rows each, rows >= 3 H / 2; "i422": H rows each, rows >= 2 H; "i444": rows >= 3 H;
    * semi-planar -- interleaved pairs from row H at ``pitch``: "nv12" (U, V) / "nv21" (V, U), H / 2 rows; "nv16" (U, V), H rows;
    * packed -- "yuyv" (Y0 U Y1 V) / "uyvy" (U Y0 V Y1), pitch >= 2 W, rows >= H.

    Bad extents raise ValueError."""
    H, W = int(H), int(W)
    if layout not in YUV_LAYOUTS:
        raise ValueError("yuv_planes: layout must be one of %s, got %r" % (", ".join(sorted(YUV_LAYOUTS)), layout))
    fmt, kind = YUV_LAYOUTS[layout]
    sx, sy = {"yuv420": (1, 1), "yuv422": (1, 0), "yuv444": (0, 0)}[fmt]
    if H < 1 or W < 1 or (sy and H % 2) or (sx and W % 2):
        raise ValueError("yuv_planes: %s needs even %s, got (%d, %d)" % (layout, "H and W" if sy else "W", H, W))
    if getattr(surfaces, "ndim", None) != 3:
        raise ValueError("yuv_planes: surfaces must be [n, rows, pitch], got shape %s" % (tuple(getattr(surfaces, "shape", ())),))
    if "uint8" not in str(surfaces.dtype):
        raise ValueError("yuv_planes: surfaces must be uint8, got %s" % (surfaces.dtype,))
    n, rows, pitch = (int(s) for s in surfaces.shape)
    ch, cw = H >> sy, W >> sx
    if hasattr(surfaces, "stride"):                    # torch: element strides of uint8 = bytes
        sn, sr, sp = (int(s) for s in surfaces.stride())
    else:
        sn, sr, sp = (int(s) for s in surfaces.strides)
    if sp != 1 and pitch > 1:
        raise ValueError("yuv_planes: the bytes of a surface row must be adjacent (stride %d)" % sp)

    def view(offset, shape, strides):
        """bytes [offset + f * sn + r * strides[0] + c * strides[1]] of the surfaces' storage"""
        if hasattr(surfaces, "as_strided"):            # torch: a view, never a copy
            return surfaces.as_strided((n,) + shape, (sn,) + strides, surfaces.storage_offset() + offset)
        import numpy as np
        if not surfaces.flags.c_contiguous:
            raise ValueError("yuv_planes: NumPy surfaces must be C-contiguous")
        return np.lib.stride_tricks.as_strided(surfaces.reshape(-1)[offset:], (n,) + shape, (sn,) + strides,
                                               writeable=surfaces.flags.writeable)

    def need(ok, what):
        if not ok:
            raise ValueError("yuv_planes: surfaces [%d, %d, %d] do not hold %d x %d %s (%s)" % (n, rows, pitch, H, W, layout, what))

    if kind == "packed":
        need(rows >= H and pitch >= 2 * W, "rows >= H, pitch >= 2 W")
        y0, u0, v0 = {"yuyv": (0, 1, 3), "uyvy": (1, 0, 2)}[layout]
        return (view(y0, (H, W), (sr, 2)), view(u0, (H, cw), (sr, 4)), view(v0, (H, cw), (sr, 4)))
    need(pitch >= W, "pitch >= W")
    y = view(0, (H, W), (sr, 1))
    if kind == "semi":
        need(rows >= H + ch and pitch >= 2 * cw, "rows >= H + chroma rows")
        first, second = view(H * sr, (ch, cw), (sr, 2)), view(H * sr + 1, (ch, cw), (sr, 2))
        return (y, second, first) if layout == "nv21" else (y, first, second)
    # planar: the chroma planes are packed behind the luma rows at their own pitch, so the surface rows must be adjacent
    cp = pitch if fmt == "yuv444" else pitch // 2
    need(sr == pitch, "planar layouts need adjacent surface rows")
    need(cp >= cw and rows * pitch >= H * pitch + 2 * ch * cp, "rows >= %s" % {"yuv420": "3 H / 2", "yuv422": "2 H", "yuv444": "3 H"}[fmt])
    first, second = view(H * pitch, (ch, cw), (cp, 1)), view(H * pitch + ch * cp, (ch, cw), (cp, 1))
    return (y, second, first) if layout == "yv12" else (y, first, second)
