"""uint8 frames for the gray pass without a GPU: the refusals (before any torch or GPU work), the six *_u8 symbols, the byte
accounting, and the host side of the new entry points -- argument validation and the host-pointer forms' staging of H * W * n BYTES
-- as a stand-alone program (tests/gray_bytes_host_main.cpp, also for the float32-frame families and the refusal table) built with the library's host side under ASan + UBSan."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT

U8 = ("silent_pyramid_u8", "silent_pyramid_u8_dev", "silent_gray_pass_u8", "silent_gray_pass_u8_dev", "silent_gray_keypoints_u8",
      "silent_gray_keypoints_u8_dev")


@pytest.mark.parametrize("kwargs", [dict(frame_dtype="int8"), dict(frame_dtype="float16"), dict(frame_dtype=None), dict(frame_dtype=8),
                                    dict(frame_dtype="u8"), dict(frame_dtype="uint8", mode="rgb"),
                                    dict(frame_dtype="uint8", accumulation="float64"), dict(frame_dtype="int8", mode="rgb"),
                                    dict(frame_dtype="int8", accumulation="float64")])
def test_pipeline_refuses_bad_frame_dtype_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match="frame_dtype"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def test_check_frame_dtype():
    from pysilent_amd import _runtime
    assert _runtime.check_frame_dtype("float32") == "float32" and _runtime.check_frame_dtype("uint8") == "uint8"
    assert _runtime.check_frame_dtype("uint8", "gray", "float32") == "uint8"
    assert _runtime.check_frame_dtype("float32", "rgb", "float64") == "float32"     # (uint8 off: nothing of it is refused)
    for args in (("int8",), ("float16",), (None,), (1,), ("uint8", "rgb"), ("uint8", "gray", "float64")):
        with pytest.raises(ValueError, match="frame_dtype"):
            _runtime.check_frame_dtype(*args)
    with pytest.raises(ValueError, match="mode 'gray'"):
        _runtime.check_frame_dtype("uint8", "rgb")
    with pytest.raises(ValueError, match="float64"):
        _runtime.check_frame_dtype("uint8", "gray", "float64")
    # the name is checked first: an unknown name is reported as such whatever else is wrong
    with pytest.raises(ValueError, match="must be 'float32' or 'uint8'"):
        _runtime.check_frame_dtype("int8", "rgb", "float64")


def test_uint8_frames_are_never_converted():
    """frame_dtype="uint8" passes the frames as they are: anything that is not uint8 is refused, not widened or narrowed."""
    import numpy as np
    from pysilent_amd import _runtime
    for bad in (np.zeros((1, 4, 4, 1), np.float32), np.zeros((1, 4, 4, 1), np.int8), np.zeros((1, 4, 4, 1), np.uint16)):
        with pytest.raises(ValueError, match="uint8"):
            _runtime._require_uint8(bad)
    _runtime._require_uint8(np.zeros((1, 4, 4, 1), np.uint8))
    with pytest.raises(TypeError):
        _runtime._require_uint8([[1, 2]])


def test_uint8_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    byte, vp = ctypes.POINTER(ctypes.c_uint8), ctypes.c_void_p
    n_args = dict(zip(U8, (5, 6, 12, 14, 20, 21)))
    for name in U8:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
        sig = _lib._SIGNATURES[name]
        assert len(sig) == n_args[name], name
        assert sig[0] is vp and sig[1] is vp and sig[2] is byte and sig[3] is ctypes.c_int, name     # ctx, plan, frames, n_frames
        # the same arguments as the float32-frame entry point behind the frames pointer
        twin = {"silent_pyramid_u8": "silent_pyramid", "silent_pyramid_u8_dev": "silent_pyramid_dev",
                "silent_gray_keypoints_u8": "silent_gray_keypoints", "silent_gray_keypoints_u8_dev": "silent_gray_keypoints_dev"}.get(name)
        if twin:
            assert sig[3:] == _lib._SIGNATURES[twin][3:], name
    for name in ("silent_gray_pass_u8", "silent_gray_pass_u8_dev"):
        sig = _lib._SIGNATURES[name]
        assert sig[8] is vp and sig[9] is vp and sig[10] is vp and sig[11] is ctypes.c_int      # pyr, cs_out, end_out (void*), maps_f16
    dev = _lib._SIGNATURES["silent_gray_pass_u8_dev"]
    assert dev[12] is ctypes.c_uint and dev[13] is vp and dev[:12] == _lib._SIGNATURES["silent_gray_pass_u8"]     # parts, stream
    assert _lib.ABI_VERSION == 5
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    assert "#define SILENT_ABI_VERSION 5" in src
    for name in U8:
        assert "const uint8_t* frames" in src[src.index("int " + name + "("):][:200], name
    p = _lib.byte_ptr(0x1001)
    assert isinstance(p, byte) and ctypes.cast(p, vp).value == 0x1001 and _lib.byte_ptr(None) is None


def test_library_exports_the_uint8_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in U8:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


def _accounting_pipeline(hw, frame_dtype, K=4, n_levels=3):
    """The byte-accounting state of a gray LineEndPipeline without its constructor (which needs a device): the attributes the
    *_bytes_per_frame methods and launch_summary read.  tests/test_gray_uint8.py asserts the same on constructed pipelines."""
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom.from_image import classic_levels
    p = LineEndPipeline.__new__(LineEndPipeline)
    p.mode, p.channels, p.frame_shape, p.crop_px, p.n_orient = "gray", 1, (hw[0], hw[1], 1), None, K
    p.frame_px = sum(l[6] * l[7] for l in classic_levels(hw, 2.0, n_levels))
    p.storage, p.accumulation, p.frame_dtype = "float32", "float32", frame_dtype
    p.torch = None            # (close() / __del__ then have nothing to do)
    return p


def test_byte_accounting_counts_one_byte_per_frame_pixel():
    h, w = 150, 316
    a, b = _accounting_pipeline((h, w), "float32"), _accounting_pipeline((h, w), "uint8")
    assert a.algorithmic_bytes_per_frame() == 4 * (h * w + 2 * a.frame_px) + 4 * a.frame_px * 5      # (the float32 count is unchanged)
    assert b.algorithmic_bytes_per_frame() == a.algorithmic_bytes_per_frame() - 3 * h * w
    assert a.pyramid_bytes_per_frame() == 4 * (h * w + a.frame_px)
    assert b.pyramid_bytes_per_frame() == a.pyramid_bytes_per_frame() - 3 * h * w
    assert b.filter_bytes_per_frame() == a.filter_bytes_per_frame()
    assert "uint8 frames" in b.launch_summary() and "uint8" not in a.launch_summary()
    assert b.dominant_kernel_name() == a.dominant_kernel_name() == "gray_stream_kernel<4,"


needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def run_driver(family, *args):
    """tests/gray_bytes_host_main.cpp + the library's host side (silent_unity.hip, -DSILENT_HOST_ONLY) as one executable under
    -fsanitize=address,undefined (build.py, build_host_driver: "u8", "u8x3" or "f32"), run as a child process -- nothing of it is loaded
    into Python: exit status 0 and no sanitizer report; returns its output."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    # (alloc_dealloc_mismatch: the host shim's operator delete is free(); the same options as the other host-side sanitizer runs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:alloc_dealloc_mismatch=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([B.build_host_driver(family)] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "AddressSanitizer" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]
    return p.stdout


@needs_hipcc
def test_u8_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Every *_u8 entry point in host and _dev form on 40 x 57 frames that are heap blocks of exactly n * H * W bytes, and the status
    codes of the ABI.  No sanitizer report, one "ok" line."""
    assert "gray uint8 host main ok" in run_driver("u8")


@needs_hipcc
def test_float32_entry_points_on_the_host_side_under_asan_and_ubsan():
    """The same for silent_pyramid, silent_gray_pass[_parts | _h], silent_gray_line_end and silent_gray_keypoints on float32 frames
    (heap blocks of exactly 4 * n * H * W bytes)."""
    assert "gray float32 host main ok" in run_driver("f32")


@needs_hipcc
def test_every_single_fault_is_refused_with_the_recorded_status_and_message():
    """name | case | status | silent_last_error of every (entry point, single fault) of the 23 entry points against
    tests/golden/gray_refusals.txt, recorded before the entry points shared their bodies.  Single faults only: the ABI promises no
    order among simultaneous ones."""
    got = "".join(run_driver(f, "--refusals") for f in ("f32", "u8", "u8x3")).splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "gray_refusals.txt")).read().splitlines()
    assert len({l.split(" | ")[0] for l in want}) == 23
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
