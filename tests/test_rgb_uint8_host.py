"""Packed uint8 colour frames for 3-channel plans (rgb_frame_dtype="uint8", silent_pyramid_rgb8[_dev]) without a GPU: the keyword's
refusals (before any torch or GPU work), the two symbols beside their *_u8 twins, the byte accounting, what the test frames of
tests/rgb_uint8_frames.py can see (each mistake a byte loader can make moves the oracle's pyramid beyond conftest.assert_close), and
the host side of the entry points -- argument validation, the refusal table, the host form's staging of exactly n * H * W * 3 bytes --
as a stand-alone program (tests/rgb8_host_main.cpp) built with the library's host side under ASan + UBSan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import err_bound as eb
import rgb_uint8_frames as rf
import silent_oracle as so
from conftest import ROOT, assert_close

RGB8 = ("silent_pyramid_rgb8", "silent_pyramid_rgb8_dev")


# ----------------------------------------------------------------------------- the keyword

@pytest.mark.parametrize("kwargs", [dict(rgb_frame_dtype="uint16"), dict(rgb_frame_dtype="float16"), dict(rgb_frame_dtype=None),
                                    dict(rgb_frame_dtype=8), dict(rgb_frame_dtype="UINT8"),
                                    dict(rgb_frame_dtype="uint8", mode="gray"),
                                    dict(rgb_frame_dtype="uint8", frame_dtype="uint8"),
                                    dict(rgb_frame_dtype="uint8", frame_dtype="uint16"),
                                    dict(rgb_frame_dtype="uint8", frame_channels=3),
                                    dict(rgb_frame_dtype="uint8", frame_layout="strided"),
                                    dict(rgb_frame_dtype="bytes", mode="gray", frame_dtype="uint8")])
def test_pipeline_refuses_bad_rgb_frame_dtype_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("mode", "rgb")
    with pytest.raises(ValueError, match="rgb_frame_dtype"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def test_check_rgb_frame_dtype():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_dtype
    assert chk("float32") == "float32" and chk("uint8") == "uint8" and chk("uint8", "rgb", "float32", 1, "packed") == "uint8"
    # the default changes nothing, whatever the other four say (they keep their own checks)
    for mode in ("gray", "rgb"):
        for fd in ("float32", "uint8", "uint16"):
            for fc in (1, 3):
                for fl in ("packed", "strided"):
                    assert chk("float32", mode, fd, fc, fl) == "float32"
    for args in (("uint16",), (None,), (8,), ("u8",), ("uint8", "gray"), ("uint8", "rgb", "uint8"), ("uint8", "rgb", "float32", 3),
                 ("uint8", "rgb", "float32", 1, "strided")):
        with pytest.raises(ValueError, match="rgb_frame_dtype"):
            chk(*args)
    with pytest.raises(ValueError, match="mode 'rgb'"):
        chk("uint8", "gray")
    with pytest.raises(ValueError, match="frame_dtype='uint8'"):
        chk("uint8", "rgb", "uint8")
    with pytest.raises(ValueError, match="frame_channels=3"):
        chk("uint8", "rgb", "float32", 3)
    with pytest.raises(ValueError, match="frame_layout='strided'"):
        chk("uint8", "rgb", "float32", 1, "strided")
    # the name is checked first: a bad name is reported as such whatever else is wrong
    with pytest.raises(ValueError, match="must be 'float32' or 'uint8'"):
        chk("uint16", "gray", "uint8", 3, "strided")


def test_the_pinned_refusals_of_mode_rgb_keep_their_texts():
    """frame_dtype / frame_channels / frame_layout on mode "rgb" are refused as before, in the older checks' own words."""
    from pysilent_amd.pipeline import LineEndPipeline
    for kwargs, text in ((dict(frame_dtype="uint8"), r"frame_dtype='uint8' is for mode 'gray' \(the RGB kernels read float32 frames\)"),
                         (dict(frame_dtype="uint8", frame_channels=3), r"frame_channels=3 is for mode 'gray'"),
                         (dict(frame_dtype="uint8", frame_layout="strided"), r"frame_dtype='uint8' is for mode 'gray'")):
        with pytest.raises(ValueError, match=text):
            LineEndPipeline((64, 96), batch=1, mode="rgb", **kwargs)


# ----------------------------------------------------------------------------- the ABI

def test_rgb8_symbols_are_declared_bound_and_exported_with_their_u8_twins_signatures():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    byte = ctypes.POINTER(ctypes.c_uint8)
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()

    def prototype(name):
        """The argument list of ``name`` in the header, whitespace collapsed."""
        at = src.index("int " + name + "(")
        return " ".join(src[at + len("int " + name):src.index(";", at)].split())

    for name in RGB8:
        twin = name.replace("_rgb8", "_u8")
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[twin], name
        assert _lib._SIGNATURES[name][2] is byte, name
        assert prototype(name) == prototype(twin), name
        assert "const uint8_t* frames" in prototype(name), name
    assert _lib.ABI_VERSION == 5
    assert "#define SILENT_ABI_VERSION 5" in src


def test_library_exports_the_rgb8_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in RGB8:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


# ----------------------------------------------------------------------------- accounting

def _accounting_pipeline(hw, frame_dtype, n_levels):
    """The byte-accounting state of an RGB LineEndPipeline without its constructor (which needs a device), config 3's maps (line_end
    and orient kept, no value map)."""
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom.from_image import classic_levels
    p = LineEndPipeline.__new__(LineEndPipeline)
    p.mode, p.channels, p.frame_shape, p.crop_px = "rgb", 3, (hw[0], hw[1], 3), None
    p.frame_px = sum(l[6] * l[7] for l in classic_levels(hw, 2.0, n_levels))
    p.storage, p.accumulation, p.frame_dtype = "float32", "float32", frame_dtype
    p.orient_map, p.value_map, p.torch = True, False, None
    return p


def test_byte_accounting_counts_one_byte_per_frame_element():
    h, w = 1080, 1920
    f32, u8 = _accounting_pipeline((h, w), "float32", 6), _accounting_pipeline((h, w), "uint8", 6)
    px = f32.frame_px
    assert f32.algorithmic_bytes_per_frame() == 4 * (h * w * 3 + 2 * px * 3) + 4 * px * 6          # (the float32 count is unchanged)
    assert u8.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 3 * h * w * 3
    assert f32.pyramid_bytes_per_frame() == 4 * 3 * (h * w + px)
    assert u8.pyramid_bytes_per_frame() == 3 * h * w + 4 * 3 * px
    assert u8.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    # the byte model of config 3 (32 x 1080p, 6 levels): frame read 24.88 -> 6.22 MB, step 157.6 -> 138.9 MB, walk launch 58.1 -> 39.4 MB
    mb = lambda b: round(b / 1e6, 1)
    assert (round(4 * h * w * 3 / 1e6, 2), round(h * w * 3 / 1e6, 2)) == (24.88, 6.22)
    assert (mb(f32.algorithmic_bytes_per_frame()), mb(u8.algorithmic_bytes_per_frame())) == (157.6, 138.9)
    assert (mb(f32.pyramid_bytes_per_frame()), mb(u8.pyramid_bytes_per_frame())) == (58.1, 39.4)
    assert "uint8 frames read in place" in u8.launch_summary() and "uint8" not in f32.launch_summary()
    assert u8.dominant_kernel_name() == f32.dominant_kernel_name()
    u8.crop_px = f32.crop_px = 1000
    assert u8.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 3 * 1000 * 3


# ----------------------------------------------------------------------------- what the test frames can see

H, W = 24, 34            # 3 W mod 4 = 2: every odd row starts 2 bytes off the dword grid


def test_the_frames_carry_the_ramp_and_the_corner_bytes():
    frames = rf.batch(2, H, W)
    assert frames.dtype == np.uint8 and frames.shape == (2, H, W, 3)
    for f in range(2):
        for y in (0, H - 1):
            for x in (0, W - 1):
                assert tuple(frames[f, y, x]) == (0, 255, 128)
    assert frames[1, 5, 7, 2] == (3 * 7 + 2 + 7 * 5) % 256 and frames[1, 11, 30, 0] == (3 * 30 + 7 * 11) % 256
    assert len(np.unique(frames[0])) > 200


@pytest.fixture(scope="module")
def correct_pyramid():
    frames = rf.batch(2, H, W)
    return frames, [so.classic_pyramid(f, 2.0, 2) for f in rf.widened(frames)]


def _beyond_assert_close(got, want, what):
    """True when conftest.assert_close, with the rounding bound of the zoom, refuses ``got`` for ``want`` on some level."""
    for l, (g, w) in enumerate(zip(got, want)):
        try:
            assert_close(g.astype(np.float32), w, 1e-5, scale=255.0, what="%s level %d" % (what, l), bound=eb.zoom(w))
        except AssertionError:
            return True
    return False


def test_the_oracle_accepts_the_correct_widening(correct_pyramid):
    frames, want = correct_pyramid
    again = [so.classic_pyramid(f, 2.0, 2) for f in frames.astype(np.float64).astype(np.float32)]
    for f in range(2):
        assert not _beyond_assert_close(again[f], want[f], "correct widening, frame %d" % f)


@pytest.mark.parametrize("name", sorted(rf.MISTAKES))
def test_the_frames_separate_each_mistake_from_the_correct_widening(correct_pyramid, name):
    """The oracle's pyramid of the frames a mistaken loader would see differs from that of the correct widening by more than
    assert_close allows -- on the frame where the mistake acts (frame 1 for the frame stride, both frames otherwise)."""
    frames, want = correct_pyramid
    seen = rf.MISTAKES[name](frames)
    assert seen.shape == frames.shape and seen.dtype == np.float32
    for f in ((1,) if name == "float-sized frame stride" else (0, 1)):
        got = so.classic_pyramid(seen[f], 2.0, 2)
        assert _beyond_assert_close(got, want[f], "%s, frame %d" % (name, f)), "%s is invisible on frame %d" % (name, f)


# ----------------------------------------------------------------------------- the host side under the sanitizers

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@needs_hipcc
def test_rgb8_entry_points_on_the_host_side_under_asan_and_ubsan():
    """tests/rgb8_host_main.cpp + the library's host side (silent_unity.hip, -DSILENT_HOST_ONLY) as one executable under
    -fsanitize=address,undefined (build.py, build_host_driver("rgb8")), run as a child process -- nothing of it is loaded into Python:
    both forms on 40 x 57 x 3 frames that are a heap block of exactly n * H * W * 3 bytes, for a classic and a crop plan; the host
    form's staged bytes are the batch and the poisoned arena behind them is untouched; the status codes and the order of the shared
    checks.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb8 host main ok" in run_driver("rgb8")


@needs_hipcc
def test_every_single_fault_of_the_rgb8_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb8", "--refusals").strip().split("\n")
    want = open(os.path.join(ROOT, "tests", "golden", "rgb8_refusals.txt")).read().strip().split("\n")
    assert len(want) == 12 and {l.split(" | ")[0] for l in want} == set(RGB8)
    assert got == want
    single = [l for l in want if "single-channel plan" in l]
    assert len(single) == 2 and all(" | -4 | " in l and "silent_pyramid_u8x3" in l for l in single)


@needs_hipcc
def test_the_existing_refusal_goldens_are_reproduced_unchanged():
    """The entry points that existed before share launch_pyramid with the new ones: their refusal tables are still the recorded ones."""
    from test_gray_uint8_host import run_driver
    for families, golden in ((("f32", "u8", "u8x3"), "gray_refusals.txt"), (("view",), "gray_view_refusals.txt"),
                             (("u16",), "gray_u16_refusals.txt")):
        got = "".join(run_driver(f, "--refusals") for f in families).strip().split("\n")
        want = open(os.path.join(ROOT, "tests", "golden", golden)).read().strip().split("\n")
        assert got == want, golden
