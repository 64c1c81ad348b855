"""CPU reference of silent_gray_keypoints' tail (test helper), composed from the oracle's own functions: the reference graph
recognition_testing.py:75-90 restricted to one input channel, on a K-channel end map --
    color = pad_inwards(end, pad); value = value_from_color(color)
    selection: value = value_from_color(nms3x3(top_value_points(color, p, value)))        (SURVEY 8d config 3's tail)
    rows = max_value_indices_region(value) per level, as (level, y, x, 0), row-major sorted."""
import numpy as np

import silent_oracle as so


def gray_tail(end_levels, pad=2, selection=True, top_percent=0.1, regions=None):
    """end_levels: one [h, w, K] float32 end map per level of ONE frame (unpadded).  Returns (rows int64 [n, 4], value maps,
    peak-value maps) -- the maps per level as [h, w] float32 (peak maps None without selection)."""
    rows, values, peaks = [], [], []
    for l, e in enumerate(end_levels):
        e = np.asarray(e, np.float32)[None]
        h, w = e.shape[1:3]
        color = so.pad_inwards(e, [[0, 0], [pad, pad], [pad, pad], [0, 0]])
        value = so.value_from_color(color)
        values.append(value[0, :, :, 0])
        v = value
        if selection:
            v = so.value_from_color(so.nms3x3(so.top_value_points(color, top_percent, value), "product"))
            peaks.append(v[0, :, :, 0])
        else:
            peaks.append(None)
        rh, rw = regions[l] if regions is not None else (max(h // 2, 1), max(w // 2, 1))
        r = so.max_value_indices_region(None, (1, rh, rw, 1), v)
        r[:, 0] = l
        rows.append(r)
    return np.concatenate(rows).astype(np.int64).reshape(-1, 4), values, peaks
