"""uint16 frames for the gray pass (frame_dtype="uint16", the silent_*_u16 and silent_*_view16 entry points) without a GPU: the
argument checks and refusals (before any torch or GPU work), the gray_entry names, frame_view_of on uint16 arrays, the twelve symbols,
the byte accounting, and the host side of the new entry points -- every single fault's status and message
(tests/golden/gray_u16_refusals.txt), and the host-pointer forms' staging of exactly `span` bytes -- as a stand-alone program
(tests/gray_u16_host_main.cpp) built with the library's host side under ASan + UBSan and run as a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

PACKED = ("silent_pyramid_u16", "silent_pyramid_u16_dev", "silent_gray_pass_u16", "silent_gray_pass_u16_dev",
          "silent_gray_keypoints_u16", "silent_gray_keypoints_u16_dev")
VIEW16 = tuple(n.replace("_u16", "_view16") for n in PACKED)
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


# ------------------------------------------------------------------------------------------ argument checks
def test_check_frame_dtype_takes_uint16():
    from pysilent_amd import _runtime
    cfd = _runtime.check_frame_dtype
    assert "uint16" in _runtime.FRAME_DTYPES and cfd("uint16") == "uint16" and cfd("uint16", "gray", "float32") == "uint16"
    with pytest.raises(ValueError, match="frame_dtype='uint16' is for mode 'gray'"):
        cfd("uint16", "rgb")
    with pytest.raises(ValueError, match="frame_dtype='uint16' does not combine with accumulation='float64'"):
        cfd("uint16", "gray", "float64")
    # the older cases keep their wording
    with pytest.raises(ValueError, match="frame_dtype='uint8' is for mode 'gray'"):
        cfd("uint8", "rgb")
    for bad in ("int16", "uint32", "UINT16", 16, None):
        with pytest.raises(ValueError, match="must be 'float32' or 'uint8' or 'uint16'"):
            cfd(bad, "rgb", "float64")


def test_check_frame_layout_and_channels_with_uint16():
    from pysilent_amd import _runtime
    cfl, cfc = _runtime.check_frame_layout, _runtime.check_frame_channels
    assert cfl("strided", "gray", "uint16", "float32") == "strided" and cfl("packed", "gray", "uint16") == "packed"
    with pytest.raises(ValueError, match="mode 'gray'"):
        cfl("strided", "rgb", "uint16")
    with pytest.raises(ValueError, match="float64"):
        cfl("strided", "gray", "uint16", "float64")
    with pytest.raises(ValueError, match="frame_layout='strided' needs frame_dtype='uint8' or 'uint16'"):
        cfl("strided", "gray", "float32")
    assert cfc(1, "gray", "uint16") == 1
    with pytest.raises(ValueError, match="frame_channels=3 needs frame_dtype='uint8'"):
        cfc(3, "gray", "uint16")


@pytest.mark.parametrize("kwargs,match", [(dict(mode="rgb"), "mode 'gray'"), (dict(accumulation="float64"), "float64"),
                                          (dict(frame_channels=3), "frame_channels=3"),
                                          (dict(frame_layout="strided", accumulation="float64"), "float64"),
                                          (dict(frame_layout="pitched"), "frame_layout")])
def test_pipeline_refuses_before_any_gpu_work(kwargs, match):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match=match):
        LineEndPipeline((64, 96), batch=1, frame_dtype="uint16", **kwargs)


def test_plan_methods_refuse_before_touching_the_frames():
    from pysilent_amd import _runtime
    plan = _runtime.PyramidPlan.__new__(_runtime.PyramidPlan)
    plan.frame_shape, plan.accumulation, plan.handle = (6, 8, 1), "float64", None
    calls = (lambda **kw: plan.run(None, **kw), lambda **kw: plan.gray_pass(None, None, None, **kw),
             lambda **kw: plan.gray_keypoints(None, None, None, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="float64"):
            call(frame_dtype="uint16")
    plan.accumulation = "float32"
    for call in calls:
        with pytest.raises(ValueError, match="frame_channels=3"):
            call(frame_dtype="uint16", frame_channels=3)
    plan.frame_shape = (6, 8, 3)
    with pytest.raises(ValueError, match="mode 'gray'"):
        plan.run(None, frame_dtype="uint16")


def test_uint16_frames_are_never_converted():
    from pysilent_amd import _runtime
    for bad in (np.zeros((1, 4, 4, 1), np.float32), np.zeros((1, 4, 4, 1), np.int16), np.zeros((1, 4, 4, 1), np.uint8),
                np.zeros((1, 4, 4, 1), np.dtype(np.uint16).newbyteorder())):
        with pytest.raises(ValueError, match="uint16"):
            _runtime._require_narrow(bad, "uint16")
    _runtime._require_narrow(np.zeros((1, 4, 4, 1), np.uint16), "uint16")
    with pytest.raises(TypeError):
        _runtime._require_narrow([[1, 2]], "uint16")


def test_gray_entry_names():
    from pysilent_amd import _lib
    ge = _lib.gray_entry
    assert ge("gray_pass", "uint16") == ("gray_pass_u16", _lib.short_ptr, _lib.void_ptr, (0,))
    assert ge("gray_pass", "uint16", 1, "float16", True, 1) == ("gray_pass_u16", _lib.short_ptr, _lib.void_ptr, (1, 1))
    assert ge("gray_pass", "uint16", 1, "float16", True, 2, frame_layout="strided") == ("gray_pass_view16", _lib.view16_ptr, _lib.void_ptr, (1, 2))
    assert ge("gray_pass", "uint16", frame_layout="strided") == ("gray_pass_view16", _lib.view16_ptr, _lib.void_ptr, (0,))
    assert ge("gray_keypoints", "uint16") == ("gray_keypoints_u16", _lib.short_ptr, _lib.void_ptr, ())
    assert ge("gray_keypoints", "uint16", dev=True, frame_layout="strided") == ("gray_keypoints_view16", _lib.view16_ptr, _lib.void_ptr, ())
    assert ge("pyramid", "uint16")[0] == "pyramid_u16" and ge("pyramid", "uint16", frame_layout="strided")[0] == "pyramid_view16"
    # the older names keep their answers
    assert ge("gray_pass", "uint8", 3, "float16", True, 1) == ("gray_pass_u8x3", _lib.byte_ptr, _lib.void_ptr, (1, 1))
    assert ge("gray_pass", "uint8", frame_layout="strided")[:2] == ("gray_pass_view", _lib.view_ptr) and ge("gray_pass")[0] == "gray_pass"
    v = _lib.view16_ptr((4096, 1, 8, 7680, 1 << 33)).contents
    assert (v.data, v.pixel_stride, v.row_stride, v.frame_stride) == (4096, 8, 7680, 1 << 33)
    assert _lib.view16_ptr(None) is None and _lib.short_ptr(None) is None
    p = _lib.short_ptr(0x1002)
    assert isinstance(p, ctypes.POINTER(ctypes.c_uint16)) and ctypes.cast(p, ctypes.c_void_p).value == 0x1002


# ------------------------------------------------------------------------------------------ frame_view_of
def test_frame_view_of_uint16_views():
    from pysilent_amd._runtime import frame_view_of
    n, H, W, pitch = 3, 10, 14, 32
    p010 = np.zeros((n, H * 3 // 2, pitch), np.uint16)
    base = p010.ctypes.data
    assert frame_view_of(p010[:, :H, :W], 1) == (base, 1, 2, 2 * pitch, 2 * pitch * H * 3 // 2)
    assert frame_view_of(p010[:, :H, :W, None], 1, "uint16") == (base, 1, 2, 2 * pitch, 2 * pitch * H * 3 // 2)
    rgba = np.zeros((n, H, W, 4), np.uint16)
    assert frame_view_of(rgba[..., 1], 1) == (rgba.ctypes.data + 2, 1, 8, 8 * W, 8 * W * H)
    assert frame_view_of(rgba[..., 1:2], 1) == (rgba.ctypes.data + 2, 1, 8, 8 * W, 8 * W * H)
    wide = np.zeros((n, H, 2 * W), np.uint16)
    assert frame_view_of(wide[:, :, ::2], 1) == (wide.ctypes.data, 1, 4, 4 * W, 4 * W * H)
    big = np.zeros((n, 23, 41), np.uint16)
    assert frame_view_of(big[:, 7:7 + H, 5:5 + W], 1) == (big.ctypes.data + 2 * (7 * 41 + 5), 1, 2, 82, 2 * 23 * 41)
    packed = np.zeros((n, H, W), np.uint16)
    assert frame_view_of(packed, 1) == (packed.ctypes.data, 1, 2, 2 * W, 2 * W * H)
    assert frame_view_of(packed[::2], 1) == (packed.ctypes.data, 1, 2, 2 * W, 4 * W * H)
    # axes of length 1 carry no stride of their own: the smallest valid one
    assert frame_view_of(packed[:1], 1)[2:] == (2, 2 * W, 2 * W * H)
    assert frame_view_of(rgba[:1, :1, :1, 0], 1)[1:] == (1, 2, 2, 2)
    # torch CPU tensors: element strides become byte strides
    import torch
    t = torch.from_numpy(p010)
    assert frame_view_of(t[:, :H, :W], 1) == (base, 1, 2, 2 * pitch, 2 * pitch * H * 3 // 2)


def test_frame_view_of_uint16_refuses():
    from numpy.lib.stride_tricks import as_strided
    from pysilent_amd._runtime import frame_view_of
    n, H, W = 2, 6, 8
    u16 = np.zeros((n, H, W), np.uint16)
    for bad, ch, what in ((u16.astype(np.int16), 1, "uint8 or uint16"), (u16.astype(np.float32), 1, "uint8 or uint16"),
                          (u16.astype(np.dtype(np.uint16).newbyteorder()), 1, "uint8 or uint16"),
                          (u16[::-1], 1, "frame stride"), (u16[:, ::-1], 1, "row stride"), (u16[:, :, ::-1], 1, "pixel stride"),
                          (np.broadcast_to(u16[:1], (n, H, W)), 1, "frame stride 0"), (np.broadcast_to(u16[:, :1], (n, H, W)), 1, "row stride 0"),
                          (np.broadcast_to(u16[:, :, :1], (n, H, W)), 1, "pixel stride 0"),
                          (u16, 3, "one channel"), (np.zeros((n, H, W, 3), np.uint16), 1, "expected"), (u16[0], 1, "expected"),
                          (u16[:0], 1, "empty")):
        with pytest.raises(ValueError, match=what):
            frame_view_of(bad, ch)
    with pytest.raises(ValueError, match="takes uint8 frames"):
        frame_view_of(u16, 1, "uint8")
    with pytest.raises(ValueError, match="takes uint16 frames"):
        frame_view_of(u16.astype(np.uint8), 1, "uint16")
    with pytest.raises(ValueError, match="frame_dtype must be"):
        frame_view_of(u16, 1, "float32")
    base = np.zeros(4096, np.uint16)
    for strides in ((2 * H * W, 2 * W - 2, 2), (2 * H * W - 2, 2 * W, 2)):           # overlapping rows / frames
        with pytest.raises(ValueError, match="overlap"):
            frame_view_of(as_strided(base, (n, H, W), strides), 1)
    odd = as_strided(base.view(np.uint8)[:2 * 4000].view(np.uint16), (n, H, W), (2 * H * W + 1, 2 * W, 2))     # an odd frame stride
    with pytest.raises(ValueError, match="even"):
        frame_view_of(odd, 1)
    with pytest.raises(TypeError):
        frame_view_of([[[1]]], 1, "uint16")


# ------------------------------------------------------------------------------------------ step_host, byte accounting
def _accounting_pipeline(hw, frame_dtype):
    from test_gray_uint8_host import _accounting_pipeline as make
    return make(hw, frame_dtype)


def test_byte_accounting_counts_two_bytes_per_frame_pixel():
    h, w = 150, 316
    a, b = _accounting_pipeline((h, w), "float32"), _accounting_pipeline((h, w), "uint16")
    assert b.algorithmic_bytes_per_frame() == a.algorithmic_bytes_per_frame() - 2 * h * w
    assert b.pyramid_bytes_per_frame() == a.pyramid_bytes_per_frame() - 2 * h * w
    assert b.filter_bytes_per_frame() == a.filter_bytes_per_frame()
    assert "uint16 frames" in b.launch_summary() and "uint16" not in a.launch_summary()
    assert "uint8 frames" in _accounting_pipeline((h, w), "uint8").launch_summary()
    assert b.dominant_kernel_name() == a.dominant_kernel_name() == "gray_stream_kernel<4,"


def test_step_host_refuses_other_dtypes_without_a_gpu():
    """step_host of a uint16 pipeline checks shape, residence and dtype before it touches a stream or a device buffer."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    p = _accounting_pipeline((12, 16), "uint16")
    p.torch, p.batch, p.frame_layout = torch, 2, "packed"
    for wrong in (np.float32, np.uint8, np.int16, np.int32):
        with pytest.raises(ValueError, match="step_host of a frame_dtype='uint16' pipeline takes uint16 host frames"):
            LineEndPipeline.step_host(p, np.zeros((2, 12, 16, 1), wrong))
    with pytest.raises(ValueError, match="host frames of shape"):
        LineEndPipeline.step_host(p, np.zeros((2, 12, 15, 1), np.uint16))
    p8 = _accounting_pipeline((12, 16), "uint8")
    p8.torch, p8.batch = torch, 2
    with pytest.raises(ValueError, match="step_host of a frame_dtype='uint8' pipeline takes uint8 host frames"):
        LineEndPipeline.step_host(p8, np.zeros((2, 12, 16, 1), np.uint16))
    p.torch = p8.torch = None


# ------------------------------------------------------------------------------------------ symbols
def test_u16_symbols_are_declared_bound_and_exported_with_their_u8_twins_argument_lists():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()

    def prototype(name):
        at = src.index("int " + name + "(")
        return " ".join(src[at + len("int " + name):src.index(";", at)].split())

    for name in PACKED:
        twin = name.replace("_u16", "_u8")
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        sig, tsig = _lib._SIGNATURES[name], _lib._SIGNATURES[twin]
        assert sig[2] is ctypes.POINTER(ctypes.c_uint16) and sig[:2] + sig[3:] == tsig[:2] + tsig[3:], name
        assert prototype(name) == prototype(twin).replace("const uint8_t* frames", "const uint16_t* frames"), name
    for name in VIEW16:
        twin = name.replace("_view16", "_u8")
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        sig, tsig = _lib._SIGNATURES[name], _lib._SIGNATURES[twin]
        assert sig[2] is ctypes.POINTER(_lib.FrameView16) and sig[:2] + sig[3:] == tsig[:2] + tsig[3:], name
        assert prototype(name) == prototype(twin).replace("const uint8_t* frames", "const silent_frame_view16* frames"), name
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src
    at = src.index("typedef struct silent_frame_view16 {")
    fields = [" ".join(l.split(";")[0].split()) for l in src[at:src.index("} silent_frame_view16;", at)].split("\n")[1:] if ";" in l]
    assert fields == ["const uint16_t* data", "int64_t pixel_stride", "int64_t row_stride", "int64_t frame_stride"]
    assert [(n, t) for n, t in _lib.FrameView16._fields_] == [("data", ctypes.c_void_p), ("pixel_stride", ctypes.c_int64),
                                                              ("row_stride", ctypes.c_int64), ("frame_stride", ctypes.c_int64)]
    assert ctypes.sizeof(_lib.FrameView16) == 32 and ctypes.sizeof(_lib.FrameView) == 40


def test_library_exports_the_u16_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in PACKED + VIEW16:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


# ------------------------------------------------------------------------------------------ the host side under the sanitizers
@needs_hipcc
def test_u16_entry_points_on_the_host_side_under_asan_and_ubsan():
    """tests/gray_u16_host_main.cpp + the library's host side as one executable under -fsanitize=address,undefined, run as a child
    process: the twelve entry points on nine layouts (packed, pitched P010 luma, a window, every second element, one channel of 16-bit
    RGBA, every second frame, single frames), each batch in a heap block of exactly `span` bytes -- a host form that stages one byte
    more is an ASan error -- and the status codes.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "gray u16 host main ok" in run_driver("u16")


@needs_hipcc
def test_every_single_fault_of_the_u16_entry_points_is_refused_with_the_recorded_status_and_message():
    """Status and silent_last_error of every (entry point, single fault) against tests/golden/gray_u16_refusals.txt: what the *_u8 /
    *_view twins refuse (under the new names, the text saying "uint16 frames") and the new refusals -- an odd frames or data address,
    an odd stride."""
    from test_gray_uint8_host import run_driver
    got = run_driver("u16", "--refusals").strip().split("\n")
    want = open(os.path.join(ROOT, "tests", "golden", "gray_u16_refusals.txt")).read().strip().split("\n")
    assert got == want
    rows = [l.split(" | ") for l in got if not l.startswith("#")]
    assert len(rows) == 228 and {r[0] for r in rows} == set(PACKED + VIEW16)
    assert all(r[2] in ("-1", "-4") and r[3].startswith(r[0].replace("_dev", "") + ": ") for r in rows)      # nothing passes, every message names its entry
    for case, status, count in (("frames at an odd address", "-1", 6), ("data at an odd address", "-1", 6), ("pixel_stride odd", "-1", 6),
                                ("row_stride odd", "-1", 6), ("frame_stride odd", "-1", 6), ("pixel_stride 1", "-1", 6),
                                ("frame_stride 2^63 - 2 (a span of 2^63 bytes or more)", "-1", 6), ("3-channel plan", "-4", 12),
                                ("ACCUM_F64 plan", "-4", 12)):
        hits = [r for r in rows if r[1] == case]
        assert len(hits) == count and all(r[2] == status and "uint16 frames" in r[3] for r in hits), case
