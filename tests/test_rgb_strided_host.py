"""Strided uint8 colour views for 3-channel plans (rgb_frame_layout="strided", silent_pyramid_rgb8_view[_dev]) without a GPU: the
keyword's refusals (before any torch or GPU work), the two symbols, what the views of tests/rgb_strided_views.py can see (each mistake
a strided loader can make moves the oracle's pyramid beyond conftest.assert_close), and the host side of the entry points --
argument validation, the refusal table, the host form's staging of exactly `span` bytes, and the walk loader's address function
enumerated over whole launches -- as a stand-alone program (tests/rgb8_view_host_main.cpp) built with the library's host side under
ASan + UBSan and run as a child process."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import err_bound as eb
import rgb_strided_views as rv
import rgb_uint8_frames as rf
import silent_oracle as so
from conftest import ROOT, assert_close

VIEW = ("silent_pyramid_rgb8_view", "silent_pyramid_rgb8_view_dev")
STRIDED = dict(rgb_frame_dtype="uint8", rgb_frame_layout="strided")


# ----------------------------------------------------------------------------- the keyword

@pytest.mark.parametrize("kwargs", [dict(rgb_frame_layout="pitched"), dict(rgb_frame_layout=None), dict(rgb_frame_layout=1),
                                    dict(rgb_frame_layout="STRIDED"),
                                    dict(rgb_frame_layout="strided"),                                   # float32 colour frames
                                    dict(rgb_frame_layout="strided", rgb_frame_dtype="float32"),
                                    dict(rgb_frame_layout="strided", mode="gray", frame_dtype="uint8"),
                                    dict(rgb_frame_layout="strided", mode="gray", frame_dtype="uint8", frame_layout="strided")])
def test_pipeline_refuses_bad_rgb_frame_layout_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("mode", "rgb")
    with pytest.raises(ValueError, match="rgb_frame_layout"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def test_check_rgb_frame_layout():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_layout
    assert chk("packed") == "packed" and chk("strided", "rgb", "uint8") == "strided"
    assert chk("strided", "rgb", "uint8", "float32", 1, "packed") == "strided"
    # the default changes nothing, whatever the others say (they keep their own checks)
    for mode in ("gray", "rgb"):
        for rd in ("float32", "uint8"):
            for fd in ("float32", "uint8", "uint16"):
                for fc in (1, 3):
                    for fl in ("packed", "strided"):
                        assert chk("packed", mode, rd, fd, fc, fl) == "packed"
    for args, text in ((("strided", "gray", "uint8"), "is for mode 'rgb'"),
                       (("strided", "rgb", "float32"), "needs rgb_frame_dtype='uint8'"),
                       (("strided", "rgb", "uint8", "uint8"), "does not combine with frame_dtype='uint8'"),
                       (("strided", "rgb", "uint8", "uint16"), "does not combine with frame_dtype='uint16'"),
                       (("strided", "rgb", "uint8", "float32", 3), "does not combine with frame_channels=3"),
                       (("strided", "rgb", "uint8", "float32", 1, "strided"), "does not combine with frame_layout='strided'")):
        with pytest.raises(ValueError, match="rgb_frame_layout='strided' " + text):
            chk(*args)
    # the name is checked first: a bad name is reported as such whatever else is wrong
    for bad in ("pitched", None, 3, "Strided"):
        with pytest.raises(ValueError, match="must be 'packed' or 'strided'"):
            chk(bad, "gray", "float32", "uint8", 3, "strided")


def test_the_older_refusals_keep_their_texts():
    """frame_layout="strided" beside rgb_frame_dtype="uint8" goes on raising its own message, and so does frame_layout="strided" on
    mode "rgb" alone."""
    from pysilent_amd import _runtime
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match=r"rgb_frame_dtype='uint8' does not combine with frame_layout='strided' \(packed frames only\)"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_dtype="uint8", frame_layout="strided")
    with pytest.raises(ValueError, match=r"rgb_frame_dtype='uint8' does not combine with frame_layout='strided' \(packed frames only\)"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_dtype="uint8", frame_layout="strided", rgb_frame_layout="strided")
    with pytest.raises(ValueError, match=r"frame_layout='strided' is for mode 'gray' \(the RGB kernels read packed float32 frames\)"):
        _runtime.check_frame_layout("strided", "rgb", "uint8")


def test_frame_view_of_refuses_what_the_strided_colour_run_refuses():
    """PyramidPlan.run(rgb_frame_layout="strided") passes its frames through frame_view_of(frames, 3, "uint8"): another channel stride,
    a stride below its bound (overlapping, broadcast, flipped) and another dtype are ValueErrors; the kinds of the tests are views."""
    from pysilent_amd._runtime import frame_view_of
    frames = rf.batch(2, 12, 10)
    for kind in rv.KINDS:
        parent = rv.place(kind, frames, 0)
        view = rv.as_numpy(parent, kind, 2, 12, 10)
        assert np.array_equal(view, frames)
        _, off, sf, sr, sp = rv.layout(kind, 2, 12, 10)
        assert frame_view_of(view, 3, "uint8") == (parent.ctypes.data + off, 3, sp, sr, sf), kind
    planar = np.zeros((2, 3, 12, 10), np.uint8).transpose(0, 2, 3, 1)            # channel stride 120
    bgr = frames[..., ::-1]                                                       # channel stride -1
    for bad, text in ((planar, "adjacent bytes"), (bgr, "adjacent bytes"), (np.broadcast_to(frames[:1], frames.shape), "positive"),
                      (frames[:, ::-1], "positive"), (np.lib.stride_tricks.as_strided(frames, frames.shape, (360, 30, 2, 1)), "overlap"),
                      (frames.astype(np.float32), "uint8"), (frames.astype(np.uint16), "uint8"), (frames[..., :2], "shape")):
        with pytest.raises(ValueError, match=text):
            frame_view_of(bad, 3, "uint8")


# ----------------------------------------------------------------------------- the ABI

def test_view_symbols_are_declared_bound_and_exported_with_the_view_twins_signatures():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()

    def prototype(name):
        at = src.index("int " + name + "(")
        return " ".join(src[at + len("int " + name):src.index(";", at)].split())

    for name in VIEW:
        twin = name.replace("_rgb8_view", "_view")
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[twin], name
        assert _lib._SIGNATURES[name][2] is _lib._wp, name
        assert prototype(name) == prototype(twin), name
        assert "const silent_frame_view* frames" in prototype(name), name
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src
    assert "MAY be loaded and dropped" in src          # the difference to the single-channel view entry points is in the header


def test_library_exports_the_view_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in VIEW:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


def test_launch_summary_and_byte_accounting_of_a_strided_colour_pipeline():
    """The summary says "read in place from a strided view"; the bytes counted are the pixel bytes of the packed uint8 pipeline (the
    bytes between the pixels of a view are not part of the algorithm's traffic)."""
    from test_rgb_uint8_host import _accounting_pipeline
    packed, strided = _accounting_pipeline((1080, 1920), "uint8", 6), _accounting_pipeline((1080, 1920), "uint8", 6)
    strided.rgb_frame_layout = "strided"
    assert "read in place from a strided view" in strided.launch_summary() and "strided" not in packed.launch_summary()
    assert strided.launch_summary().startswith(packed.launch_summary())
    for fn in ("algorithmic_bytes_per_frame", "pyramid_bytes_per_frame", "filter_bytes_per_frame"):
        assert getattr(strided, fn)() == getattr(packed, fn)(), fn


# ----------------------------------------------------------------------------- what the views can see

H, W = 24, 34


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


@pytest.mark.parametrize("kind", rv.KINDS)
def test_the_views_carry_the_batch_under_both_fills(correct_pyramid, kind):
    frames, want = correct_pyramid
    for fill in rv.FILLS:
        parent = rv.place(kind, frames, fill)
        assert parent.size == rv.layout(kind, 2, H, W)[0] and rv.layout(kind, 2, H, W)[1] + rv.span(kind, 2, H, W) <= parent.size
        seen = rv.truth(parent, kind, 2, H, W)
        assert np.array_equal(seen, rf.widened(frames)) and np.array_equal(rv.as_numpy(parent, kind, 2, H, W), frames)
        if kind != "packed":
            assert np.count_nonzero(parent == fill) >= parent.size - frames.size     # (bytes between the pixels keep the fill)
    assert not _beyond_assert_close([so.classic_pyramid(f, 2.0, 2) for f in seen][1], want[1], "truth")


@pytest.mark.parametrize("name", sorted(rv.MISTAKES))
def test_the_views_separate_each_mistake_from_the_truth(correct_pyramid, name):
    """On every kind of view where the mistake changes an address, the oracle's pyramid of what a mistaken loader would see differs
    from the true one by more than assert_close allows, under at least one of the two fills (a byte that is not the view's but
    changes the result shows under 0x00 or under 0xFF) -- on the frame where the mistake acts (frame 1 for the frame stride)."""
    frames, want = correct_pyramid
    assert rv.VISIBLE_ON[name]
    for kind in rv.VISIBLE_ON[name]:
        shown = False
        for fill in rv.FILLS:
            seen = rv.MISTAKES[name](rv.place(kind, frames, fill), kind, 2, H, W)
            assert seen.shape == frames.shape and seen.dtype == np.float32
            frames_hit = (1,) if name == "frame stride taken as packed" else (0, 1)
            shown = shown or all(_beyond_assert_close(so.classic_pyramid(seen[f], 2.0, 2), want[f], "%s, %s" % (name, kind)) for f in frames_hit)
        assert shown, "%s is invisible on %s" % (name, kind)


# ----------------------------------------------------------------------------- the host side under the sanitizers

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@needs_hipcc
def test_view_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Both forms on 40 x 57 views (BGRA, an odd-pitch BGR with a gap between its frames, a packed view) whose data is a heap block of
    exactly `span` bytes, for a classic and a crop plan; the host form's staged bytes are the span and the poisoned arena behind them
    is untouched; the status codes and the order of the checks.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb8 view host main ok" in run_driver("rgb8_view")


@needs_hipcc
def test_every_single_fault_of_the_view_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb8_view", "--refusals").strip().split("\n")
    want = open(os.path.join(ROOT, "tests", "golden", "rgb8_view_refusals.txt")).read().strip().split("\n")
    assert len(want) == 28 and {l.split(" | ")[0] for l in want} == set(VIEW)
    assert got == want
    assert all(l.split(" | ")[3].startswith("silent_pyramid_rgb8_view: ") for l in want)
    channels = [l for l in want if " | channels " in l]
    assert len(channels) == 4 and all(" | -1 | " in l and "view channels must be 3" in l for l in channels)
    single = [l for l in want if "single-channel plan" in l]
    assert len(single) == 2 and all(" | -4 | " in l and "silent_pyramid_view)" in l for l in single)
    # check_view's refusals under the new name, in check_view's words
    gray = open(os.path.join(ROOT, "tests", "golden", "gray_view_refusals.txt")).read()
    for l in want:
        text = l.split(" | ")[3].split(": ", 1)[1]
        if "stride" in text or "spans" in text:
            assert "silent_pyramid_view: " + text in gray, text


@needs_hipcc
def test_the_packed_colour_refusal_golden_is_reproduced_unchanged():
    """silent_pyramid_rgb8[_dev] share their checks with the view forms: their refusal table is still the recorded one."""
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb8", "--refusals").strip().split("\n")
    assert got == open(os.path.join(ROOT, "tests", "golden", "rgb8_refusals.txt")).read().strip().split("\n")


E5 = math.e ** .5


def _address_plans():
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    return [((40, 8), classic_levels((40, 8), 2.0, 2)), ((64, 66), classic_levels((64, 66), 2.0, 3)),
            ((135, 241), classic_levels((135, 241), 2.0, 4)), ((270, 482), reference_levels((270, 482), (61, 45), 2.0))]


@needs_hipcc
@pytest.mark.parametrize("which", range(4), ids=["classic-40x8", "classic-64x66", "classic-135x241", "crops-270x482"])
def test_every_address_of_the_walk_loader_lies_inside_the_span_and_covers_the_crops(which):
    """--addresses: w3_view_load -- the function pyramid_walk3_kernel forms its view loads with -- for every block, chunk, row, lane and
    load slot of the plan's launch on two frames, for each kind of view: no access outside [0, span), none misaligned for its width,
    and every channel byte of every pixel of the walk plans' crops is among the bytes touched."""
    from test_gray_uint8_host import run_driver
    hw, levels = _address_plans()[which]
    out = run_driver("rgb8_view", "--addresses", str(hw[0]), str(hw[1]), str(len(levels)), *[str(int(v)) for l in levels for v in l])
    lines = [l for l in out.strip().split("\n") if l]
    assert len(lines) == len(rv.KINDS) - 1, out                      # (a packed view does not take the view loader)
    for l in lines:
        f = l.split(" | ")
        assert f[0] == "%d x %d" % hw and f[4] == "outside 0" and f[5] == "misaligned 0" and f[6].endswith("missing 0"), l
        assert int(f[6].split()[1]) > 0 and int(f[3].split()[1]) > 0, l
    if which == 3:
        assert all("plans 2 " in l for l in lines)
