"""The Python refusals of the four YUV-family colour sources as WHOLE strings: every refusal of nv12_frames_of / p010_frames_of /
yuv_frames_of / yuv16_frames_of on the bad inputs of the per-format suites (NumPy arrays, N = 2, H = 24, W = 34), and every refusal
of check_rgb_frame_format per format family -- exception type and full text, recorded in tests/golden/rgb_source_python_refusals.txt.
The per-format suites match substrings; this one keeps a shared message builder from drifting by a word.  The inputs are built from
np.zeros parents with fixed slicing, so the strides a message quotes are the same on every run; no message quotes an address.

    python tests/test_rgb_source_messages.py --record      # rewrites the golden file from the code as it is
"""
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgb_source_python_refusals.txt")
N, H, W = 2, 24, 34
M = np.eye(3, dtype=np.float32)


def _pair(dtype):
    """(y, uv): pitched views [N, H, W] and [N, H / 2, W / 2, 2] inside zero parents (row pitch W + 6 elements, 3 / 1 spare rows)."""
    y = np.zeros((N, H + 3, W + 6), dtype)[:, :H, :W]
    uv = np.zeros((N, H // 2 + 1, (W + 6) // 2, 2), dtype)[:, :H // 2, :W // 2]
    return y, uv


def _triple(dtype):
    """(y, u, v): pitched planar 4:2:0 views inside zero parents (u and v with equal strides, in parents of their own)."""
    y = np.zeros((N, H + 3, W + 6), dtype)[:, :H, :W]
    u = np.zeros((N, H // 2 + 1, W // 2 + 5), dtype)[:, :H // 2, :W // 2]
    v = np.zeros((N, H // 2 + 1, W // 2 + 5), dtype)[:, :H // 2, :W // 2]
    return y, u, v


def _pair_cases(name, call, dtype, others):
    y, uv = _pair(dtype)
    bad = [("uv_reversed_pairs", (y, uv[:, :, :, ::-1])), ("y_reversed_columns", (y[:, :, ::-1], uv)), ("y_float32", (y.astype(np.float32), uv))]
    bad += [("y_%s" % np.dtype(t).name, (y.astype(t), uv)) for t in others]
    bad += [("uv_int16", (y, uv.astype(np.int16))), ("uv_one_frame", (y, uv[:1])), ("y_23_rows", (y[:, :23], uv)), ("y_reversed_rows", (y[:, ::-1], uv)),
            ("y_broadcast", (np.broadcast_to(y[:1], y.shape), uv)), ("three_planes", (y, uv, uv)), ("one_plane", y), ("a_list_for_uv", (y, [1, 2]))]
    return [("%s/%s" % (name, k), (lambda p=p: call(p))) for k, p in bad]


def _triple_cases(name, call, dtype, others):
    y, u, v = _triple(dtype)
    st = np.lib.stride_tricks.as_strided
    bad = [("two_planes", (y, u)), ("one_plane", y), ("y_float32", (y.astype(np.float32), u, v)), ("v_signed", (y, u, v.astype(np.dtype(dtype).name[1:])))]
    bad += [("y_%s" % np.dtype(t).name, (y.astype(t), u, v)) for t in others]
    bad += [("u_one_frame", (y, u[:1], v)), ("v_5_columns", (y, u, v[:, :, :5])), ("y_23_rows", (y[:, :23], u, v)),
            ("v_contiguous", (y, u, np.ascontiguousarray(v))), ("y_reversed_columns", (y[:, :, ::-1], u, v)),
            ("uv_reversed_rows", (y, u[:, ::-1], v[:, ::-1])), ("y_broadcast", (np.broadcast_to(y[:1], y.shape), u, v)),
            ("a_list_for_v", (y, u, [1, 2]))]
    if np.dtype(dtype).itemsize == 2:       # a row stride of an odd number of bytes (never dereferenced: the refusal reads strides only)
        bad.append(("y_odd_row_stride", (st(y, y.shape, (y.strides[0], y.strides[1] + 1, 2)), u, v)))
    return [("%s/%s" % (name, k), (lambda p=p: call(p))) for k, p in bad]


def cases():
    """[(id, callable)]: every callable raises."""
    from pysilent_amd import _runtime as rt
    out = _pair_cases("nv12_frames_of", lambda p: rt.nv12_frames_of(p, (H, W), M, 16.0), np.uint8, ())
    out += _pair_cases("p010_frames_of", lambda p: rt.p010_frames_of(p, (H, W), M, 64.0, 512.0, 10), np.uint16, (np.uint8,))
    y, uv = _pair(np.uint16)
    out.append(("p010_frames_of/depth_8", lambda: rt.p010_frames_of((y, uv), (H, W), M, 64.0, 512.0, 8)))
    out += _triple_cases("yuv_frames_of", lambda p: rt.yuv_frames_of(p, (H, W), "yuv420", M, 16.0), np.uint8, ())
    t8 = _triple(np.uint8)
    out.append(("yuv_frames_of/yuv444_of_420_planes", lambda: rt.yuv_frames_of(t8, (H, W), "yuv444", M, 16.0)))
    out.append(("yuv_frames_of/fmt_yuv", lambda: rt.yuv_frames_of(t8, (H, W), "yuv", M, 16.0)))
    out += _triple_cases("yuv16_frames_of", lambda p: rt.yuv16_frames_of(p, (H, W), "yuv420p10", M, 64.0, 512.0), np.uint16, (np.uint8,))
    t16 = _triple(np.uint16)
    out.append(("yuv16_frames_of/yuv444p10_of_420_planes", lambda: rt.yuv16_frames_of(t16, (H, W), "yuv444p10", M, 64.0, 512.0)))
    out.append(("yuv16_frames_of/fmt_yuv420", lambda: rt.yuv16_frames_of(t16, (H, W), "yuv420", M, 64.0, 512.0)))
    # check_rgb_frame_format: per format the refusals in their order (mode, the four combinations, extents), then the bad names
    ok = ("rgb", "float32", "packed", "float32", 1, "packed")
    for fmt in ("nv12",) + tuple(rt.P010_DEPTHS) + tuple(rt.YUV_SHIFTS) + tuple(sorted(rt.YUV16_FORMATS)):
        combos = [("gray", (fmt, "gray")), ("rgb_frame_dtype", (fmt, "rgb", "uint8")), ("rgb_frame_layout", (fmt, "rgb", "float32", "strided")),
                  ("frame_dtype", (fmt, "rgb", "float32", "packed", "uint8")), ("frame_channels", (fmt, "rgb", "float32", "packed", "float32", 3)),
                  ("frame_layout", (fmt, "rgb", "float32", "packed", "float32", 1, "strided")),
                  ("all_wrong_gray", (fmt, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))),
                  ("all_wrong_rgb", (fmt, "rgb", "uint8", "strided", "uint8", 3, "strided", (3, 5))),
                  ("all_wrong_float32", (fmt, "rgb", "float32", "strided", "uint8", 3, "strided", (3, 5)))]
        combos += [("hw_%dx%d" % hw, (fmt,) + ok + (hw,)) for hw in ((25, 34), (24, 33), (25, 33), (0, 34), (24, 0))]
        for k, a in combos:
            out.append(("check_rgb_frame_format/%s/%s" % (fmt, k), (lambda a=a: rt.check_rgb_frame_format(*a))))
    for bad in ("yuv", None, 3, "Nv12", "yuv420p", "yuv420p14", "yuv440p10", "yuv420p16msb"):
        out.append(("check_rgb_frame_format/name/%r" % (bad,), (lambda b=bad: rt.check_rgb_frame_format(b, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5)))))
    return out


def replay():
    """One line per case: id, exception type and whole message (or "no refusal": 4:2:2 / 4:4:4 accept odd extents), tab-separated."""
    lines = []
    for name, f in cases():
        try:
            f()
            lines.append("%s\tno refusal" % name)
        except Exception as e:              # noqa: BLE001 -- the type is what is recorded
            text = str(e)
            assert "\n" not in text and "\t" not in text, name
            lines.append("%s\t%s\t%s" % (name, type(e).__name__, text))
    return lines


def test_every_python_refusal_of_the_four_sources_is_the_recorded_string():
    want = open(GOLDEN).read().splitlines()
    got = replay()
    assert len(got) == len(want) and len(got) > 300
    for g, w in zip(got, want):
        assert g == w
    # the record holds refusals of every function and both exception types
    for head in ("nv12_frames_of/", "p010_frames_of/", "yuv_frames_of/", "yuv16_frames_of/", "check_rgb_frame_format/"):
        assert sum(1 for w in want if w.startswith(head) and "\tno refusal" not in w) >= 10
    assert sum(1 for w in want if "\tTypeError\t" in w) == 4


if __name__ == "__main__":
    if "--record" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        with open(GOLDEN, "w") as fh:
            fh.write("\n".join(replay()) + "\n")
        print("wrote %s" % GOLDEN)
