"""Strided uint8 frames for the gray pass (frame_layout="strided", the silent_*_view entry points) without a GPU: the refusals (before
any torch or GPU work), frame_view_of on NumPy views, the six symbols, and the host side of the new entry points -- every single fault's
status and message, and the host-pointer forms' staging of exactly `span` bytes -- as a stand-alone program
(tests/gray_view_host_main.cpp) built with the library's host side under ASan + UBSan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

VIEW = ("silent_pyramid_view", "silent_pyramid_view_dev", "silent_gray_pass_view", "silent_gray_pass_view_dev",
        "silent_gray_keypoints_view", "silent_gray_keypoints_view_dev")
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


# ------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kwargs", [dict(frame_layout="pitched"), dict(frame_layout=None), dict(frame_layout=1),
                                    dict(frame_layout="strided", mode="rgb", frame_dtype="float32"),
                                    dict(frame_layout="strided", frame_dtype="float32"),
                                    dict(frame_layout="strided", accumulation="float64", frame_dtype="float32")])
def test_pipeline_refuses_bad_frame_layout_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("frame_dtype", "uint8")
    with pytest.raises(ValueError, match="frame_layout"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def test_check_frame_layout():
    from pysilent_amd import _runtime
    cfl = _runtime.check_frame_layout
    assert cfl("packed") == "packed"
    for mode in ("gray", "rgb"):
        for fd in ("float32", "uint8"):
            for acc in ("float32", "float64"):
                assert cfl("packed", mode, fd, acc) == "packed"
    assert cfl("strided", "gray", "uint8", "float32") == "strided"
    with pytest.raises(ValueError, match="mode 'gray'"):
        cfl("strided", "rgb", "uint8")
    with pytest.raises(ValueError, match="frame_dtype='uint8'"):
        cfl("strided", "gray", "float32")
    with pytest.raises(ValueError, match="frame_dtype='uint8'"):
        cfl("strided")
    with pytest.raises(ValueError, match="float64"):
        cfl("strided", "gray", "uint8", "float64")
    # the name is checked first: a bad name is reported as such whatever else is wrong
    for bad in ("Strided", "", None, 0, True):
        with pytest.raises(ValueError, match="must be 'packed' or 'strided'"):
            cfl(bad, "rgb", "float32", "float64")


def test_the_older_checks_and_gray_entry_keep_their_answers():
    import inspect
    from pysilent_amd import _lib, _runtime
    assert list(inspect.signature(_runtime.check_frame_channels).parameters) == ["frame_channels", "mode", "frame_dtype", "accumulation"]
    assert list(inspect.signature(_runtime.check_frame_dtype).parameters) == ["frame_dtype", "mode", "accumulation"]
    assert list(inspect.signature(_lib.gray_entry).parameters)[:6] == ["family", "frame_dtype", "frame_channels", "storage", "dev", "parts"]
    assert _lib.gray_entry("gray_pass", "uint8", 3, "float16", True, 1) == ("gray_pass_u8x3", _lib.byte_ptr, _lib.void_ptr, (1, 1))
    assert _lib.gray_entry("gray_pass")[0] == "gray_pass" and _lib.gray_entry("gray_keypoints", "uint8")[0] == "gray_keypoints_u8"
    # the _view names: one family for both channel counts, the frames argument made from a view tuple
    for ch in (1, 3):
        assert _lib.gray_entry("gray_pass", "uint8", ch, "float16", True, 2, frame_layout="strided") == \
            ("gray_pass_view", _lib.view_ptr, _lib.void_ptr, (1, 2))
        assert _lib.gray_entry("gray_pass", "uint8", ch, frame_layout="strided") == ("gray_pass_view", _lib.view_ptr, _lib.void_ptr, (0,))
        assert _lib.gray_entry("gray_keypoints", "uint8", ch, dev=True, frame_layout="strided") == \
            ("gray_keypoints_view", _lib.view_ptr, _lib.void_ptr, ())
        assert _lib.gray_entry("pyramid", "uint8", ch, frame_layout="strided")[0] == "pyramid_view"
    v = _lib.view_ptr((4096, 3, 4, 7680, 1 << 33)).contents
    assert (v.data, v.channels, v.pixel_stride, v.row_stride, v.frame_stride) == (4096, 3, 4, 7680, 1 << 33)
    assert _lib.view_ptr(None) is None


# ------------------------------------------------------------------------------------------ frame_view_of
def test_frame_view_of_numpy_views():
    from pysilent_amd._runtime import frame_view_of
    n, H, W, pitch = 3, 10, 14, 32
    surface = np.zeros((n, H * 3 // 2, pitch), np.uint8)
    base = surface.ctypes.data
    assert frame_view_of(surface[:, :H, :W, None], 1) == (base, 1, 1, pitch, pitch * H * 3 // 2)
    assert frame_view_of(surface[:, :H, :W], 1) == (base, 1, 1, pitch, pitch * H * 3 // 2)
    bgra = np.zeros((n, H, W, 4), np.uint8)
    assert frame_view_of(bgra[..., :3], 3) == (bgra.ctypes.data, 3, 4, 4 * W, 4 * W * H)
    assert frame_view_of(bgra[..., 1:2], 1) == (bgra.ctypes.data + 1, 1, 4, 4 * W, 4 * W * H)
    yuyv = np.zeros((n, H, 2 * W), np.uint8)
    assert frame_view_of(yuyv[:, :, ::2, None], 1) == (yuyv.ctypes.data, 1, 2, 2 * W, 2 * W * H)
    big = np.zeros((n, 23, 41), np.uint8)
    assert frame_view_of(big[:, 7:7 + H, 5:5 + W], 1) == (big.ctypes.data + 7 * 41 + 5, 1, 1, 41, 23 * 41)
    bgr = np.zeros((n, 23, 41, 3), np.uint8)
    assert frame_view_of(bgr[:, 7:7 + H, 5:5 + W], 3) == (bgr.ctypes.data + (7 * 41 + 5) * 3, 3, 3, 41 * 3, 23 * 41 * 3)
    packed = np.zeros((n, H, W, 3), np.uint8)
    assert frame_view_of(packed, 3) == (packed.ctypes.data, 3, 3, 3 * W, 3 * W * H)
    assert frame_view_of(packed[::2], 3) == (packed.ctypes.data, 3, 3, 3 * W, 2 * 3 * W * H)
    # axes of length 1 carry no stride of their own: the smallest valid one
    assert frame_view_of(packed[:1], 3) == (packed.ctypes.data, 3, 3, 3 * W, 3 * W * H)
    assert frame_view_of(np.broadcast_to(np.zeros((1, H, W, 1), np.uint8), (1, H, W, 1)), 1)[2:] == (1, W, H * W)
    one = frame_view_of(bgra[:1, :1, :1, :3], 3)
    assert one[1:] == (3, 3, 3, 3)


def test_frame_view_of_refuses():
    from pysilent_amd._runtime import frame_view_of
    n, H, W = 2, 6, 8
    u8 = np.zeros((n, H, W, 3), np.uint8)
    for bad, ch, what in ((u8.astype(np.float32), 3, "uint8"), (u8.astype(np.int8), 3, "uint8"),
                          (u8[::-1], 3, "frame stride"), (u8[:, ::-1], 3, "row stride"), (u8[:, :, ::-1], 3, "pixel stride"),
                          (u8[..., ::-1], 3, "channel stride 1"),
                          (np.broadcast_to(u8[:1], (n, H, W, 3)), 3, "frame stride 0"),
                          (np.broadcast_to(u8[:, :1], (n, H, W, 3)), 3, "row stride 0"),
                          (np.broadcast_to(u8[:, :, :1], (n, H, W, 3)), 3, "pixel stride 0"),
                          (u8, 1, "expected"), (u8[..., :2], 3, "expected"), (u8[0], 3, "expected"), (u8[..., 0], 3, "expected"),
                          (u8[:0], 3, "empty")):
        with pytest.raises(ValueError, match=what):
            frame_view_of(bad, ch)
    # overlapping pixels / rows (as_strided): refused here, as the library would
    from numpy.lib.stride_tricks import as_strided
    base = np.zeros(4096, np.uint8)
    for strides in ((H * W * 3, W * 3, 2, 1), (H * W * 3, W * 3 - 1, 3, 1), (H * W * 3 - 1, W * 3, 3, 1)):
        with pytest.raises(ValueError, match="overlap"):
            frame_view_of(as_strided(base, (n, H, W, 3), strides), 3)
    for ch in (2, 0, 4, "3", 3.0, True, None):
        with pytest.raises(ValueError, match="channels must be 1 or 3"):
            frame_view_of(u8, ch)
    with pytest.raises(TypeError):
        frame_view_of([[[[1]]]], 1)


def test_plan_methods_refuse_a_bad_layout_before_touching_the_frames():
    """PyramidPlan.run / gray_pass / gray_keypoints check frame_layout with the other frame arguments, before the frames are looked at
    (the plan object here has no device behind it)."""
    from pysilent_amd import _runtime
    plan = _runtime.PyramidPlan.__new__(_runtime.PyramidPlan)
    plan.frame_shape, plan.accumulation, plan.handle = (6, 8, 1), "float32", None
    for call in (lambda **kw: plan.run(None, **kw), lambda **kw: plan.gray_pass(None, None, None, **kw),
                 lambda **kw: plan.gray_keypoints(None, None, None, **kw)):
        with pytest.raises(ValueError, match="must be 'packed' or 'strided'"):
            call(frame_dtype="uint8", frame_layout="pitched")
        with pytest.raises(ValueError, match="frame_layout='strided' needs frame_dtype='uint8'"):
            call(frame_layout="strided")
    plan.accumulation = "float64"
    with pytest.raises(ValueError, match="float64"):
        plan.run(None, frame_dtype="uint8", frame_layout="strided")


# ------------------------------------------------------------------------------------------ symbols
def test_view_symbols_are_declared_bound_and_exported_with_their_u8_twins_argument_lists():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()

    def prototype(name):
        at = src.index("int " + name + "(")
        return " ".join(src[at + len("int " + name):src.index(";", at)].split())

    for name in VIEW:
        twin = name.replace("_view", "_u8")
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        sig, tsig = _lib._SIGNATURES[name], _lib._SIGNATURES[twin]
        assert sig[2] is ctypes.POINTER(_lib.FrameView) and sig[:2] + sig[3:] == tsig[:2] + tsig[3:], name
        assert prototype(name) == prototype(twin).replace("const uint8_t* frames", "const silent_frame_view* frames"), name
    assert _lib.ABI_VERSION == 5
    assert "#define SILENT_ABI_VERSION 5" in src
    # the struct as the header declares it
    at = src.index("typedef struct silent_frame_view {")
    fields = [" ".join(l.split(";")[0].split()) for l in src[at:src.index("} silent_frame_view;", at)].split("\n")[1:] if ";" in l]
    assert fields == ["const uint8_t* data", "int channels", "int64_t pixel_stride", "int64_t row_stride", "int64_t frame_stride"]
    assert [(n, t) for n, t in _lib.FrameView._fields_] == [("data", ctypes.c_void_p), ("channels", ctypes.c_int),
                                                            ("pixel_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                                                            ("frame_stride", ctypes.c_int64)]
    assert ctypes.sizeof(_lib.FrameView) == 40


def test_library_exports_the_view_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in VIEW:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


# ------------------------------------------------------------------------------------------ the host side under the sanitizers
@needs_hipcc
def test_view_entry_points_on_the_host_side_under_asan_and_ubsan():
    """tests/gray_view_host_main.cpp + the library's host side as one executable under -fsanitize=address,undefined, run as a child
    process: the six entry points on eleven layouts (packed, pitched, YUYV luma, one channel of BGR, BGRA, odd BGR pitch, every second
    frame, single frames), each view in a heap block of exactly `span` bytes -- a host form that stages one byte more is an ASan
    error -- and the status codes.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "gray view host main ok" in run_driver("view")


@needs_hipcc
def test_every_single_fault_of_the_view_entry_points_is_refused_with_the_recorded_status_and_message():
    """Status and silent_last_error of every (entry point, single fault), for a one-channel and a three-channel strided view, against
    tests/golden/gray_view_refusals.txt: what the *_u8 twins refuse (under the _view names) and the view's own refusals -- NULL view,
    NULL data, channels other than 1 or 3, each stride one below its bound, zero and negative, a span of 2^63 bytes."""
    from test_gray_uint8_host import run_driver
    got = run_driver("view", "--refusals").strip().split("\n")
    want = open(os.path.join(ROOT, "tests", "golden", "gray_view_refusals.txt")).read().strip().split("\n")
    assert got == want
    rows = [l.split(" | ") for l in got if not l.startswith("#")]
    assert len(rows) == 288 and {r[0] for r in rows} == set(VIEW)
    assert all(r[2] in ("-1", "-4") and r[3].startswith(r[0].replace("_dev", "") + ": ") for r in rows)      # nothing passes, every message names its entry
    for case in ("view NULL", "data NULL", "channels 2", "channels 0", "pixel_stride channels - 1", "pixel_stride 0", "pixel_stride -4",
                 "row_stride one below its bound", "row_stride 0", "row_stride negative", "frame_stride one below its bound",
                 "frame_stride 0", "frame_stride negative", "frame_stride 2^63 - 1 (a span of 2^63 bytes or more)"):
        hits = [r for r in rows if r[1] == case]
        assert len(hits) == 12 and all(r[2] == "-1" for r in hits), case
