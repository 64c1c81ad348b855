"""P010 / P012 / P016 decoder surfaces as the pair of planes the RGB pyramid reads in place (LineEndPipeline(mode="rgb",
rgb_frame_format="p010"), PyramidPlan.run(rgb_frame_format="p010"))."""


def p010_planes(surfaces, H, W, chroma_row=None):
    """(y, uv) views of P010 / P012 / P016 surfaces ``surfaces`` [n, R, pitch_elements] (uint16 torch tensor or ndarray; nothing is
    copied): the luma plane y = surfaces[:, :H, :W] and the chroma plane uv [n, H / 2, W / 2, 2] of interleaved (U, V) element pairs,
    whose rows start at row ``chroma_row`` of each surface (default H: chroma directly below luma; decoders that align the luma height
    put it lower) and share the surface's pitch."""
    H, W = int(H), int(W)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("p010_planes: H and W must be even (4:2:0 chroma), got (%d, %d)" % (H, W))
    if getattr(surfaces, "ndim", None) != 3:
        raise ValueError("p010_planes: surfaces must be [n, rows, pitch_elements], got shape %s" % (tuple(getattr(surfaces, "shape", ())),))
    if "uint16" not in str(surfaces.dtype):
        raise ValueError("p010_planes: surfaces must be uint16 (one element per code value), got %s" % (surfaces.dtype,))
    c0 = H if chroma_row is None else int(chroma_row)
    n, rows, pitch = (int(s) for s in surfaces.shape)
    if c0 < H or rows < c0 + H // 2 or pitch < W:
        raise ValueError("p010_planes: surfaces [%d, %d, %d] do not hold %d x %d luma and chroma rows %d .. %d"
                         % (n, rows, pitch, H, W, c0, c0 + H // 2 - 1))
    y = surfaces[:, :H, :W]
    uv = surfaces[:, c0:c0 + H // 2, :W]
    if hasattr(uv, "unflatten"):                       # torch: a view, never a copy
        uv = uv.unflatten(2, (W // 2, 2))
    else:
        import numpy as np
        s = uv.strides
        uv = np.lib.stride_tricks.as_strided(uv, (n, H // 2, W // 2, 2), (s[0], s[1], 2 * s[2], s[2]), writeable=uv.flags.writeable)
    return y, uv
