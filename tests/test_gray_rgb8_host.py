"""Interleaved 3-channel uint8 frames for the gray pass (frame_channels=3, the silent_*_u8x3 entry points) without a GPU: the
refusals (before any torch or GPU work), the six symbols beside their *_u8 twins, the byte accounting, and the host side of the new
entry points -- argument validation and the host-pointer forms' staging of 3 * H * W * n BYTES -- as a stand-alone program
(tests/gray_bytes_host_main.cpp) built with the library's host side under ASan + UBSan."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT

U8X3 = ("silent_pyramid_u8x3", "silent_pyramid_u8x3_dev", "silent_gray_pass_u8x3", "silent_gray_pass_u8x3_dev",
        "silent_gray_keypoints_u8x3", "silent_gray_keypoints_u8x3_dev")


@pytest.mark.parametrize("kwargs", [dict(frame_channels=2), dict(frame_channels=4), dict(frame_channels="3"),
                                    dict(frame_channels=3, mode="rgb"), dict(frame_channels=3, frame_dtype="float32"),
                                    dict(frame_channels=3, accumulation="float64"), dict(frame_channels=0), dict(frame_channels=None),
                                    dict(frame_channels=2, frame_dtype="float32")])
def test_pipeline_refuses_bad_frame_channels_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("frame_dtype", "uint8")
    with pytest.raises(ValueError, match="frame_channels"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def test_check_frame_channels():
    from pysilent_amd import _runtime
    cfc = _runtime.check_frame_channels
    # 1 is the default and is always fine
    assert cfc(1) == 1
    for mode in ("gray", "rgb"):
        for fd in ("float32", "uint8"):
            for acc in ("float32", "float64"):
                assert cfc(1, mode, fd, acc) == 1
    assert cfc(3, "gray", "uint8", "float32") == 3
    for args in ((2,), (4,), ("3",), (0,), (None,), (3.0,), (True,),
                 (3, "rgb", "uint8", "float32"), (3, "gray", "float32", "float32"), (3, "gray", "uint8", "float64"), (3,)):
        with pytest.raises(ValueError, match="frame_channels"):
            cfc(*args)
    with pytest.raises(ValueError, match="mode 'gray'"):
        cfc(3, "rgb", "uint8")
    with pytest.raises(ValueError, match="frame_dtype='uint8'"):
        cfc(3, "gray", "float32")
    with pytest.raises(ValueError, match="float64"):
        cfc(3, "gray", "uint8", "float64")
    # the value is checked first: a bad count is reported as such whatever else is wrong
    with pytest.raises(ValueError, match="must be 1 or 3"):
        cfc(2, "rgb", "float32", "float64")


def test_the_older_checks_keep_their_signatures():
    """check_frame_dtype / check_storage / check_accumulation are pinned by earlier tests: same arguments, same answers."""
    import inspect
    from pysilent_amd import _runtime
    assert list(inspect.signature(_runtime.check_frame_dtype).parameters) == ["frame_dtype", "mode", "accumulation"]
    assert list(inspect.signature(_runtime.check_storage).parameters) == ["storage", "mode", "accumulation", "keypoints"]
    assert list(inspect.signature(_runtime.check_accumulation).parameters) == ["accumulation"]
    assert list(inspect.signature(_runtime.check_frame_channels).parameters) == ["frame_channels", "mode", "frame_dtype", "accumulation"]
    assert _runtime.check_frame_dtype("uint8", "gray", "float32") == "uint8"


def test_u8x3_symbols_are_declared_bound_and_exported_with_their_u8_twins_signatures():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    byte = ctypes.POINTER(ctypes.c_uint8)
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()

    def prototype(name):
        """The argument list of ``name`` in the header, whitespace collapsed."""
        at = src.index("int " + name + "(")
        return " ".join(src[at + len("int " + name):src.index(";", at)].split())

    for name in U8X3:
        twin = name.replace("_u8x3", "_u8")
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[twin], name
        assert _lib._SIGNATURES[name][2] is byte, name
        assert prototype(name) == prototype(twin), name
        assert "const uint8_t* frames" in prototype(name), name
    assert _lib.ABI_VERSION == 5
    assert "#define SILENT_ABI_VERSION 5" in src


def test_library_exports_the_u8x3_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in U8X3:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


def _accounting_pipeline(hw, frame_dtype, frame_c, K=4, n_levels=3):
    """The byte-accounting state of a gray LineEndPipeline without its constructor (which needs a device), with the attributes
    tests/test_gray_uint8_host.py sets and NO others: the accounting must follow from frame_shape[2] and frame_dtype."""
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom.from_image import classic_levels
    p = LineEndPipeline.__new__(LineEndPipeline)
    p.mode, p.channels, p.frame_shape, p.crop_px, p.n_orient = "gray", 1, (hw[0], hw[1], frame_c), None, K
    p.frame_px = sum(l[6] * l[7] for l in classic_levels(hw, 2.0, n_levels))
    p.storage, p.accumulation, p.frame_dtype = "float32", "float32", frame_dtype
    p.torch = None            # (close() / __del__ then have nothing to do)
    return p


def test_byte_accounting_counts_three_bytes_per_frame_pixel():
    h, w = 150, 316
    f32, u8, rgb8 = (_accounting_pipeline((h, w), "float32", 1), _accounting_pipeline((h, w), "uint8", 1),
                     _accounting_pipeline((h, w), "uint8", 3))
    px = f32.frame_px
    assert f32.algorithmic_bytes_per_frame() == 4 * (h * w + 2 * px) + 4 * px * 5          # (the older counts are unchanged)
    assert u8.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 3 * h * w
    assert rgb8.algorithmic_bytes_per_frame() == u8.algorithmic_bytes_per_frame() + 2 * h * w
    assert rgb8.algorithmic_bytes_per_frame() == 3 * h * w + 4 * 2 * px + 4 * px * 5       # frame 3 B/px; pyramid and maps one channel
    assert f32.pyramid_bytes_per_frame() == 4 * (h * w + px)
    assert u8.pyramid_bytes_per_frame() == h * w + 4 * px
    assert rgb8.pyramid_bytes_per_frame() == 3 * h * w + 4 * px
    assert rgb8.filter_bytes_per_frame() == u8.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    assert "uint8 frames" in rgb8.launch_summary() and "3 interleaved channels" in rgb8.launch_summary()
    assert "interleaved" not in u8.launch_summary() and "uint8" not in f32.launch_summary()
    assert rgb8.dominant_kernel_name() == u8.dominant_kernel_name() == "gray_stream_kernel<4,"
    # a crop layout reads the crop at 3 bytes per pixel
    rgb8.crop_px = u8.crop_px = 1000
    assert rgb8.algorithmic_bytes_per_frame() == u8.algorithmic_bytes_per_frame() + 2 * 1000


def test_rgb_mode_accounting_is_unchanged():
    """Mode "rgb" (3-channel float32 frames, 3-channel maps): frame_shape[2] = channels = 3 counts as before."""
    from pysilent_amd.pipeline import LineEndPipeline
    p = LineEndPipeline.__new__(LineEndPipeline)
    p.mode, p.channels, p.frame_shape, p.crop_px = "rgb", 3, (64, 96, 3), None
    p.frame_px, p.storage, p.accumulation, p.frame_dtype = 9000, "float32", "float32", "float32"
    p.orient_map, p.value_map, p.torch = True, True, None
    assert p.algorithmic_bytes_per_frame() == 4 * (64 * 96 * 3 + 2 * 9000 * 3) + 4 * 9000 * 7
    assert p.pyramid_bytes_per_frame() == 4 * 3 * (64 * 96 + 9000)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_u8x3_entry_points_on_the_host_side_under_asan_and_ubsan():
    """tests/gray_bytes_host_main.cpp + the library's host side (silent_unity.hip, -DSILENT_HOST_ONLY) as one executable under
    -fsanitize=address,undefined, run as a child process: every new entry point in host and _dev form on 40 x 57 x 3 frames that are
    heap blocks of exactly 3 * n * H * W bytes, and the status codes of the ABI.  No sanitizer report, one "ok" line.  (A program of
    its own: nothing of it is loaded into Python.)"""
    from test_gray_uint8_host import run_driver
    assert "gray rgb8 host main ok" in run_driver("u8x3")
