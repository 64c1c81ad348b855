"""Raw 8-bit Bayer mosaics for 3-channel plans (rgb_frame_format="bayer_rggb" / "bayer_grbg" / "bayer_gbrg" / "bayer_bggr",
silent_pyramid_bayer[_dev], silent_bayer_to_rgb[_dev]) without a GPU: the three statements the NumPy restatement of
tests/rgb_bayer_frames.py must pass before anything is compared with it, the keyword's refusals (before any torch or GPU work),
bayer_frames_of on every layout, the alias table, the symbols and the struct (its ctypes mirror against the C compiler's sizeof /
offsets), the byte accounting, and the host side of the entry points -- argument validation, the refusal table, the host forms'
staging of exactly the view's span, and the walk loader's address function enumerated over whole launches with the exchange of the
neighbouring columns replayed -- as a stand-alone program (tests/rgb_bayer_host_main.cpp) built with the library's host side under
ASan + UBSan and run as a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rgb_bayer_frames as bf
from conftest import ROOT
from test_rgb_nv12_host import needs_hipcc, odd_origin_crops

NAMES = ("silent_pyramid_bayer", "silent_pyramid_bayer_dev", "silent_bayer_to_rgb", "silent_bayer_to_rgb_dev")
FORMATS = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")
GOLDEN = os.path.join(ROOT, "tests", "golden")
N, H, W = 2, 24, 34


# ----------------------------------------------------------------------------- the restatement

def test_the_restatement_passes_its_three_checks():
    """A mosaic of a constant colour comes back as exactly (r, g, b) at every pixel (four patterns; 2 x 2, 3 x 2, 24 x 34, 25 x 33);
    rggb / bgr equals bggr / rgb bit for bit; every value stays in [0, 255]."""
    assert bf.checks()


def test_the_restatement_by_hand_on_a_3_x_3_frame():
    """Every neighbour of the centre exists, every neighbour of a corner is reflected: the words of the header, by hand."""
    m = np.array([[[10, 20, 30], [40, 50, 60], [70, 80, 90]]], np.uint8)
    t = bf.truth(m, "rggb", "rgb")
    # (1, 1) is a blue site of rggb: blue 50, green the cross, red the diagonals
    assert t[0, 1, 1].tolist() == [(10 + 30 + 70 + 90) * .25, (20 + 80 + 40 + 60) * .25, 50.0]
    # (0, 0) is a red site; its neighbours -1 reflect onto 1: green (40 + 40 + 20 + 20) / 4, blue 4 x 50 / 4
    assert t[0, 0, 0].tolist() == [10.0, 30.0, 50.0]
    # (0, 1) is a green site in a red row: red (10 + 30) / 2, blue (50 + 50) / 2
    assert t[0, 0, 1].tolist() == [20.0, 20.0, 50.0]
    # (2, 1): row 2 is a red row again; blue from rows 1 and 3 -> 1
    assert t[0, 2, 1].tolist() == [80.0, 80.0, 50.0]
    # (1, 2) is a green site in a blue row: blue (50 + 50) / 2 (column 3 -> 1), red (30 + 90) / 2
    assert t[0, 1, 2].tolist() == [60.0, 60.0, 50.0]
    assert np.array_equal(bf.truth(m, "rggb", "bgr"), t[..., ::-1])
    q = bf.truth(np.array([[[1, 2], [4, 7]]], np.uint8), "grbg", "rgb")         # 2 x 2: every neighbour reflected
    assert q[0, 0, 0].tolist() == [2.0, 1.0, 4.0] and q[0, 0, 1].tolist() == [2.0, (7 + 7 + 1 + 1) * .25, 4.0]
    assert q[0, 1, 0].tolist() == [2.0, (1 + 1 + 7 + 7) * .25, 4.0] and q[0, 1, 1].tolist() == [2.0, 7.0, 4.0]


def test_window_pattern_names():
    from pysilent_amd.util.zoom import BAYER_LAYOUTS, bayer_window
    assert bf.window_pattern("rggb", 3, 5) == "bggr" and bf.window_pattern("rggb", 1, 0) == "gbrg" and bf.window_pattern("grbg", 0, 1) == "rggb"
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, (1, 12, 14)).astype(np.uint8)
    for p in bf.PATTERNS:
        for y0 in range(2):
            for x0 in range(2):
                assert bayer_window("bayer_" + p, y0, x0) == "bayer_" + bf.window_pattern(p, y0, x0)
                # the interior of a window's conversion is the interior of the sensor's (the borders reflect differently)
                a = bf.truth(big, p)[:, y0 + 1:-1, x0 + 1:-1]
                b = bf.truth(np.ascontiguousarray(big[:, y0:, x0:]), bf.window_pattern(p, y0, x0))[:, 1:-1, 1:-1]
                assert np.array_equal(a, b)
    assert BAYER_LAYOUTS["BayerRG8"] == "bayer_rggb" and BAYER_LAYOUTS["BayerGR8"] == "bayer_grbg"
    assert BAYER_LAYOUTS["BayerGB8"] == "bayer_gbrg" and BAYER_LAYOUTS["BayerBG8"] == "bayer_bggr"
    assert set(BAYER_LAYOUTS.values()) == set(FORMATS)
    with pytest.raises(ValueError, match="fmt must be one of"):
        bayer_window("rggb", 0, 0)


# ----------------------------------------------------------------------------- the keyword

NAMES_APPENDED = r"'bayer_rggb' / 'bayer_grbg' / 'bayer_gbrg' / 'bayer_bggr'; util.zoom.BAYER_LAYOUTS maps the GenICam names\)$"
PIPELINE_REFUSALS = [(dict(rgb_frame_format="bayer"), NAMES_APPENDED), (dict(rgb_frame_format="bayer_rgbg"), NAMES_APPENDED),
                     (dict(rgb_frame_format="BayerRG8"), NAMES_APPENDED),
                     (dict(rgb_frame_format="bayer_rggb", mode="gray"), r"rgb_frame_format='bayer_rggb' is for mode 'rgb' \(a gray value from a mosaic"),
                     (dict(rgb_frame_format="bayer_grbg", rgb_frame_dtype="uint8"), "rgb_frame_format='bayer_grbg' does not combine with rgb_frame_dtype='uint8'"),
                     (dict(rgb_frame_format="bayer_gbrg", rgb_frame_dtype="uint8", rgb_frame_layout="strided"),
                      "rgb_frame_format='bayer_gbrg' does not combine with rgb_frame_dtype='uint8'"),
                     (dict(rgb_frame_format="bayer_bggr", hw=(1, 96)), r"rgb_frame_format='bayer_bggr' needs H and W of at least 2, got \(1, 96\)"),
                     (dict(rgb_frame_format="bayer_bggr", hw=(64, 1)), r"rgb_frame_format='bayer_bggr' needs H and W of at least 2, got \(64, 1\)"),
                     (dict(rgb_frame_format="bayer_rggb", nv12_matrix="bt601"), "rgb_frame_format='bayer_rggb' does not combine with nv12_matrix"),
                     (dict(rgb_frame_format="bayer_rggb", nv12_range="full"), "rgb_frame_format='bayer_rggb' does not combine with nv12_range='full'"),
                     (dict(rgb_frame_format="bayer_rggb", nv12_matrix=np.eye(3)), "rgb_frame_format='bayer_rggb' does not combine with nv12_matrix")]


@pytest.mark.parametrize("kwargs,text", PIPELINE_REFUSALS, ids=[str(i) for i in range(len(PIPELINE_REFUSALS))])
def test_pipeline_refuses_bad_rgb_frame_format_before_any_gpu_work(kwargs, text):
    """Each with the text of ITS refusal (the parent's unknown-name message also says "rgb_frame_format")."""
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs = dict(kwargs)
    kwargs.setdefault("mode", "rgb")
    hw = kwargs.pop("hw", (64, 96))
    with pytest.raises(ValueError, match=text):
        LineEndPipeline(hw, batch=1, **kwargs)


def test_pipeline_refuses_a_bad_order_before_any_gpu_work():
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match="nv12_order must be 'bgr' or 'rgb'"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_format="bayer_rggb", nv12_order="gbr")


def test_check_rgb_frame_format():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_format
    assert tuple(_runtime.BAYER_FORMATS) == FORMATS and _runtime.BAYER_FORMATS == dict(zip(FORMATS, range(4)))
    assert all(f[6:] == p for f, p in zip(FORMATS, bf.PATTERNS))
    assert _runtime.RGB_FRAME_FORMATS == ("interleaved", "nv12", "p010", "p012", "p016")       # (a table of its own, like YUV_SHIFTS)
    for fmt in FORMATS:
        assert chk(fmt) == fmt and chk(fmt, "rgb", hw=(25, 33)) == fmt and chk(fmt, "rgb", hw=(2, 2)) == fmt
        name = "rgb_frame_format='%s' " % fmt
        for args, text in (((fmt, "gray"), r"is for mode 'rgb' \(a gray value from a mosaic is not provided\)"),
                           ((fmt, "rgb", "uint8"), "does not combine with rgb_frame_dtype='uint8'"),
                           ((fmt, "rgb", "float32", "strided"), "does not combine with rgb_frame_layout='strided'"),
                           ((fmt, "rgb", "float32", "packed", "uint8"), "does not combine with frame_dtype='uint8'"),
                           ((fmt, "rgb", "float32", "packed", "float32", 3), "does not combine with frame_channels=3"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "strided"), "does not combine with frame_layout='strided'"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "packed", (1, 34)), r"needs H and W of at least 2, got \(1, 34\)"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "packed", (24, 1)), r"needs H and W of at least 2, got \(24, 1\)")):
            with pytest.raises(ValueError, match=name + text):
                chk(*args)
        # the order: mode, combinations, extents
        with pytest.raises(ValueError, match="is for mode 'rgb'"):
            chk(fmt, "gray", "uint8", "strided", "uint8", 3, "strided", (1, 1))
        with pytest.raises(ValueError, match="rgb_frame_dtype='uint8'"):
            chk(fmt, "rgb", "uint8", "strided", "uint8", 3, "strided", (1, 1))
        with pytest.raises(ValueError, match="rgb_frame_layout='strided'"):
            chk(fmt, "rgb", "float32", "strided", "uint8", 3, "strided", (1, 1))
    # a bad name keeps the message's beginning; one that reads like a Bayer format gets the Bayer names at the END
    begin = r"rgb_frame_format must be 'interleaved' or 'nv12', or 'p010' / 'p012' / 'p016', or 'yuv420' / 'yuv422' / 'yuv444', got "
    for bad in ("bayer", "bayer_rgbg", "BayerRG8", "Bayer_RGGB"):
        with pytest.raises(ValueError, match=begin + r".*'bayer_rggb' / 'bayer_grbg' / 'bayer_gbrg' / 'bayer_bggr'; util.zoom.BAYER_LAYOUTS maps the GenICam names\)$"):
            chk(bad, "gray", "uint8", "strided", "uint8", 3, "strided", (1, 1))
    with pytest.raises(ValueError, match=begin + r"'rggb' .*444\)$"):
        chk("rggb")


def test_check_bayer_conversion():
    from pysilent_amd._runtime import check_bayer_conversion as chk
    assert chk("bayer_rggb") == 0 and chk("bayer_rggb", nv12_order="rgb") == 1 and chk("bayer_bggr", "bt709", "limited", "bgr") == 0
    for kw, text in ((dict(nv12_matrix="bt601"), "does not combine with nv12_matrix"), (dict(nv12_matrix="bt2020"), "does not combine with nv12_matrix"),
                     (dict(nv12_matrix=np.eye(3, dtype=np.float32)), "does not combine with nv12_matrix"),
                     (dict(nv12_matrix=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]), "does not combine with nv12_matrix"),
                     (dict(nv12_range="full"), "does not combine with nv12_range='full'"), (dict(nv12_order="brg"), "nv12_order must be")):
        with pytest.raises(ValueError, match=text):
            chk("bayer_grbg", **kw)


def test_plan_run_refuses_a_matrix_or_a_range_beside_a_mosaic():
    """PyramidPlan.run checks the keyword, then the conversion keywords, before it looks at the frames or the plan's handle."""
    from pysilent_amd._runtime import PyramidPlan
    plan = PyramidPlan.__new__(PyramidPlan)
    plan.frame_shape, plan.handle = (H, W, 3), None
    m = np.zeros((N, H, W), np.uint8)
    with pytest.raises(ValueError, match="does not combine with nv12_matrix"):
        plan.run(m, rgb_frame_format="bayer_rggb", nv12_matrix="bt601")
    with pytest.raises(ValueError, match="does not combine with nv12_range='full'"):
        plan.run(m, rgb_frame_format="bayer_rggb", nv12_range="full")
    with pytest.raises(ValueError, match="rgb_frame_format='bayer_rggb' does not combine with rgb_frame_dtype='uint8'"):
        plan.run(m, rgb_frame_format="bayer_rggb", rgb_frame_dtype="uint8")
    gray = PyramidPlan.__new__(PyramidPlan)
    gray.frame_shape, gray.handle = (H, W, 1), None
    with pytest.raises(ValueError, match="rgb_frame_format='bayer_rggb' is for mode 'rgb'"):
        gray.run(m, rgb_frame_format="bayer_rggb")
    small = PyramidPlan.__new__(PyramidPlan)
    small.frame_shape, small.handle = (1, W, 3), None
    with pytest.raises(ValueError, match="needs H and W of at least 2"):
        small.run(m[:, :1], rgb_frame_format="bayer_rggb")


def test_no_new_keyword():
    import inspect
    from pysilent_amd.pipeline import LineEndPipeline
    names = list(inspect.signature(LineEndPipeline.__init__).parameters)
    assert names[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"]
    from pysilent_amd import _runtime
    assert list(inspect.signature(_runtime.PyramidPlan.run).parameters)[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"]
    assert list(inspect.signature(_runtime.bayer_to_rgb).parameters) == ["frames", "hw", "fmt", "nv12_order", "device"]
    assert inspect.signature(_runtime.bayer_to_rgb).parameters["nv12_order"].default == "bgr"


# ----------------------------------------------------------------------------- bayer_frames_of

@pytest.mark.parametrize("name", list(bf.LAYOUTS))
def test_bayer_frames_of_on_every_layout(name):
    """The view passes as it is: the struct's fields are its address and strides, nothing is converted or copied."""
    from pysilent_amd._runtime import bayer_frames_of
    s = bf.spec(name, N, H, W)
    m = bf.batch(s)
    for fill in bf.FILLS:
        parent = bf.place(s, m, fill)
        v = bf.view(s, parent)
        assert np.array_equal(v, m) and np.shares_memory(v, parent)
        mask = np.zeros(s["size"], bool)
        bf.view(s, mask)[...] = True
        assert mask.sum() == N * H * W and np.all(parent[~mask] == fill) and bf.span(s) <= s["size"] - s["offset"]
        for pattern in ("rggb", "gbrg"):
            for order in bf.ORDERS:
                for frames in (v, v[..., None]):
                    args, n, dev = bayer_frames_of(frames, (H, W), "bayer_" + pattern, order)
                    assert args == bf.struct_args(s, parent.ctypes.data, pattern, order) and n == N and not dev
    if name == "odd_window":
        assert s["shift"] == (3, 5) and s["strides"][1] == W + 12


def test_bayer_frames_of_refusals():
    from pysilent_amd._runtime import bayer_frames_of
    s = bf.spec("pitched", N, H, W)
    v = bf.view(s, bf.place(s, bf.batch(s), 0))
    for bad, text in ((v.astype(np.float32), "uint8"), (v.astype(np.int8), "uint8"), (v.astype(np.uint16), "uint8"), (v[:, :23], r"must be \[n, 24, 34\]"),
                      (v[:, :, :33], r"must be \[n, 24, 34\]"), (v[0], r"must be \[n, 24, 34\]"), (np.stack([v, v, v], -1), r"or \[n, 24, 34, 1\]"),
                      (v[:, :, ::-1], "not positive"), (v[:, ::-1], "not positive"), (v[::-1], "not positive"),
                      (np.broadcast_to(v[:1], v.shape), "overlap"), (np.broadcast_to(v[:, :1], v.shape), "overlap")):
        with pytest.raises(ValueError, match=text):
            bayer_frames_of(bad, (H, W), "bayer_rggb")
    with pytest.raises(ValueError, match="fmt must be one of bayer_rggb, bayer_grbg, bayer_gbrg, bayer_bggr"):
        bayer_frames_of(v, (H, W), "rggb")
    with pytest.raises(ValueError, match="nv12_order must be"):
        bayer_frames_of(v, (H, W), "bayer_rggb", "grb")
    with pytest.raises(ValueError, match="needs H and W of at least 2"):
        bayer_frames_of(v[:, :1], (1, W), "bayer_rggb")
    with pytest.raises(TypeError):
        bayer_frames_of([[1, 2], [3, 4]], (2, 2), "bayer_rggb")
    # one frame: the frame stride is not the view's (which NumPy leaves arbitrary) but the frame's extent
    args, n, _ = bayer_frames_of(v[:1], (H, W), "bayer_bggr", "rgb")
    assert n == 1 and args[1:] == (1, W + 13, (H - 1) * (W + 13) + W, 3, 1)


# ----------------------------------------------------------------------------- the ABI

def test_bayer_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert "const silent_bayer_frames* frames" in " ".join(src[src.index("int " + name + "("):].split(";")[0].split()), name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["silent_pyramid_bayer"] == [vp, vp, _lib._byp, i, vp]
    assert _lib._SIGNATURES["silent_pyramid_bayer_dev"] == _lib._SIGNATURES["silent_pyramid_bayer"] + [vp]
    assert _lib._SIGNATURES["silent_bayer_to_rgb"] == [vp, _lib._byp, i, i, i, vp]
    assert _lib._SIGNATURES["silent_bayer_to_rgb_dev"] == _lib._SIGNATURES["silent_bayer_to_rgb"] + [vp]
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src
    # the two statements the header owes its readers
    text = " ".join(src.replace("\n *", " ").split())
    assert "NOT OpenCV's COLOR_Bayer*2BGR" in text and "OpenCV's pattern names are shifted against the sensor's" in text


def test_library_exports_the_bayer_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


@needs_hipcc
def test_the_ctypes_struct_matches_the_c_compilers_layout():
    """sizeof(silent_bayer_frames) and the offset of every field as the host program prints them (--sizeof) against the ctypes mirror."""
    from pysilent_amd import _lib
    from test_gray_uint8_host import run_driver
    line = run_driver("rgb_bayer", "--sizeof").strip().split(" | ")
    S = _lib.BayerFrames
    assert line[0] == "sizeof %d" % ctypes.sizeof(S) and ctypes.sizeof(S) == 40
    tokens = line[1].split()
    assert tokens[0::2] == [f[0] for f in S._fields_]
    assert [int(t) for t in tokens[1::2]] == [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 32, 36]
    p = _lib.bayer_ptr((1, 2, 3, 4, 3, 1)).contents
    assert (p.data, p.pixel_stride, p.row_stride, p.frame_stride, p.pattern, p.order) == (1, 2, 3, 4, 3, 1)
    assert _lib.bayer_ptr(None) is None


# ----------------------------------------------------------------------------- the accounting

def test_launch_summary_and_byte_accounting():
    """One byte per pixel -- a third of a byte per frame element, exact; everything else is the float32 pipeline's."""
    from test_rgb_uint8_host import _accounting_pipeline
    h, w = 1080, 1920
    f32, p = _accounting_pipeline((h, w), "float32", 6), _accounting_pipeline((h, w), "float32", 6)
    p.rgb_frame_format = "bayer_grbg"
    assert "bayer_grbg mosaics read in place" in p.launch_summary() and p.launch_summary().startswith(f32.launch_summary())
    assert "1 byte per pixel" in p.launch_summary()
    assert p._frame_bytes * 3 == 1
    assert p.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 12 * h * w + h * w
    assert p.pyramid_bytes_per_frame() == f32.pyramid_bytes_per_frame() - 12 * h * w + h * w
    assert p.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    assert type(p.algorithmic_bytes_per_frame()) is int and type(p.pyramid_bytes_per_frame()) is int
    assert p.dominant_kernel_name() == f32.dominant_kernel_name()
    # the issue's figures: 32 x 1080p is 66 MB of mosaics against 796 MB of float32 frames
    assert (round(32 * h * w / 1e6), round(32 * 12 * h * w / 1e6)) == (66, 796)


# ----------------------------------------------------------------------------- the host side under the sanitizers

@needs_hipcc
def test_bayer_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Both forms of both entry points, for a classic and a crop plan of a 41 x 59 frame, on the four layouts with the mosaic in a heap
    block of exactly the view's span: the host forms stage the span byte for byte and the poisoned arena behind it is untouched; a byte
    one past the span is never read (AddressSanitizer would report it); 2 x 2 and 3 x 2 frames; one frame with a frame stride that is
    not read; status codes and the order of the checks.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb bayer host main ok" in run_driver("rgb_bayer")


@needs_hipcc
def test_every_single_fault_of_the_bayer_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb_bayer", "--refusals").strip().split("\n")
    want = open(os.path.join(GOLDEN, "bayer_refusals.txt")).read().strip().split("\n")
    assert len(want) == 2 * 23 + 2 * 19 and {l.split(" | ")[0] for l in want} == set(NAMES)
    assert got == want
    for l in want:
        name, case, status, text = l.split(" | ")
        assert text.startswith(name.replace("_dev", "") + ": "), l
        assert status == ("-4" if case in ("single-channel plan", "float64 plan") else "-1"), l
    assert sum("pattern must be 0 .. 3" in l for l in want) == 8 and sum("order must be 0 (bgr) or 1 (rgb)" in l for l in want) == 8
    assert sum("H and W of at least 2" in l for l in want) == 8 and sum("pixel_stride is below 1" in l for l in want) == 8
    assert sum("row_stride is below" in l for l in want) == 8 and sum("frame_stride is below" in l for l in want) == 12
    assert sum("NULL pointer" in l for l in want) == 2 * 4 + 2 * 3 and sum("2^63" in l for l in want) == 4
    f64 = [l for l in want if " | float64 plan | " in l]
    assert len(f64) == 2 and all("SILENT_PLAN_ACCUM_F64" in l for l in f64)      # (such a plan is single-channel: named as float64 first)
    assert sum("3-channel plans" in l for l in want) == 2
    assert sum("n_frames must be >= 1" in l for l in want) == 8 and sum("another context" in l for l in want) == 2


def _address_cases():
    import math
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    e5 = math.e ** .5
    hw, center, _ = odd_origin_crops()
    return [("packed", (40, 8), classic_levels((40, 8), 2.0, 2)), ("pitched", (64, 66), classic_levels((64, 66), 2.0, 3)),
            ("pixel_stride_2", (65, 67), classic_levels((65, 67), e5, 3)), ("odd_window", (134, 242), classic_levels((134, 242), 2.0, 4)),
            ("pitched", (136, 240), classic_levels((136, 240), e5, 4)), ("pixel_stride_2", hw, reference_levels(hw, center, 2.0)),
            ("odd_window", (480, 640), reference_levels((480, 640), (288, 192), e5))]


@needs_hipcc
@pytest.mark.parametrize("which", range(7), ids=["packed-40x8", "pitched-64x66", "pixel_stride_2-65x67-e", "odd_window-134x242", "pitched-136x240-e",
                                                 "pixel_stride_2-crops-270x482", "odd_window-reference-480x640"])
def test_every_address_of_the_walk_loader_is_a_pixel_and_every_neighbourhood_is_the_mosaics(which):
    """--addresses: w3_bayer_load -- the function pyramid_walk3_kernel forms its mosaic loads with -- for every block, chunk, row, lane
    and load slot of the plan's launch on two frames: every offset lies inside the span and is the byte of a pixel of the view, in a row
    in [0, H) that is yy - 1, yy or yy + 1 reflected; with the exchange replayed (lane j takes the columns of lanes j - 1 and j + 1
    across the load slots, w3_bayer_sums applies the edge rule), every crop pixel a ring row holds gets its own sample and the sums of
    its horizontal, vertical and diagonal neighbours as the mosaic has them; every such pixel is written; the 3 x 3 neighbourhood of
    every crop pixel is among the bytes touched."""
    from test_gray_uint8_host import run_driver
    layout, hw, levels = _address_cases()[which]
    out = run_driver("rgb_bayer", "--addresses", layout, str(hw[0]), str(hw[1]), str(len(levels)), *[str(int(v)) for l in levels for v in l])
    lines = [l for l in out.strip().split("\n") if l]
    assert len(lines) == 1, out
    f = lines[0].split(" | ")
    assert f[0] == "%s %d x %d" % ((layout,) + tuple(hw)) and f[3] == "outside 0" and f[4] == "not a pixel byte 0" and f[5] == "wrong rows 0 offsets 0", lines[0]
    t = f[6].split()
    assert int(t[2]) > 0 and t[3:] == ["wrong", "sums", "0", "unwritten", "0"], lines[0]
    assert int(f[7].split()[1]) > 0 and f[7].endswith("missing 0") and int(f[2].split()[1]) > 0, lines[0]
    if which == 5:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
        assert "plans 2 " in f[1] and int(f[8].split()[2]) >= 1, lines[0]
