"""NV12 decoder surfaces as the pair of planes the RGB pyramid reads in place (LineEndPipeline(mode="rgb",
rgb_frame_format="nv12"), PyramidPlan.run(rgb_frame_format="nv12"))."""


def nv12_planes(surfaces, H, W, chroma_row=None):
    """(y, uv) views of NV12 surfaces ``surfaces`` [n, R, pitch] (uint8 torch tensor or ndarray; nothing is copied): the luma plane
    y = surfaces[:, :H, :W] and the chroma plane uv [n, H / 2, W / 2, 2] of interleaved (U, V) pairs, whose rows start at row
    ``chroma_row`` of each surface (default H: chroma directly below luma; decoders that align the luma height put it lower) and
    share the surface's pitch."""
    H, W = int(H), int(W)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("nv12_planes: H and W must be even (4:2:0 chroma), got (%d, %d)" % (H, W))
    if getattr(surfaces, "ndim", None) != 3:
        raise ValueError("nv12_planes: surfaces must be [n, rows, pitch], got shape %s" % (tuple(getattr(surfaces, "shape", ())),))
    c0 = H if chroma_row is None else int(chroma_row)
    n, rows, pitch = (int(s) for s in surfaces.shape)
    if c0 < H or rows < c0 + H // 2 or pitch < W:
        raise ValueError("nv12_planes: surfaces [%d, %d, %d] do not hold %d x %d luma and chroma rows %d .. %d"
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
