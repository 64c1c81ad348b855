"""Raw Bayer mosaics: the names a camera gives its pixel format -> the rgb_frame_format that reads it in place."""

# GenICam PFNC names (GigE Vision, USB3 Vision) and the V4L2 / MIPI fourccs of the same 8-bit mosaics -> rgb_frame_format.  The name
# is that of the top-left 2 x 2 cell of the VIEW that is passed: a window that starts on an odd row or column of the sensor has
# another name than the sensor (bayer_window).  OpenCV's COLOR_Bayer* constants are shifted against these names (its "BayerBG" is a
# sensor's RGGB): go by the camera's pixel format, not by OpenCV's constant.
BAYER_LAYOUTS = {"BayerRG8": "bayer_rggb", "BayerGR8": "bayer_grbg", "BayerGB8": "bayer_gbrg", "BayerBG8": "bayer_bggr",
                 "RGGB": "bayer_rggb", "GRBG": "bayer_grbg", "GBRG": "bayer_gbrg", "BA81": "bayer_bggr",
                 "SRGGB8": "bayer_rggb", "SGRBG8": "bayer_grbg", "SGBRG8": "bayer_gbrg", "SBGGR8": "bayer_bggr"}

_ORDER = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")      # pattern 0 .. 3: red at (pattern >> 1, pattern & 1)


def bayer_window(fmt, y0, x0):
    """The rgb_frame_format of a window of a mosaic of format ``fmt`` that starts at row y0, column x0: an odd row offset swaps the
    rows of the 2 x 2 cell, an odd column offset its columns (mosaic[:, y0:, x0:] is read with bayer_window(fmt, y0, x0))."""
    if fmt not in _ORDER:
        raise ValueError("fmt must be one of %s, got %r" % (", ".join(_ORDER), fmt))
    return _ORDER[_ORDER.index(fmt) ^ ((int(y0) & 1) << 1) ^ (int(x0) & 1)]
