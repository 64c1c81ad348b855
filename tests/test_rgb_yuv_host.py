"""Planar and packed 8-bit YUV for 3-channel plans (rgb_frame_format="yuv420" / "yuv422" / "yuv444", silent_pyramid_yuv[_dev],
silent_yuv_to_rgb[_dev]) without a GPU: the keyword's refusals and their order (before any torch or GPU work), yuv_frames_of and
yuv_planes on every layout, the symbols and the struct (its ctypes mirror against the C compiler's sizeof / offsets), what the test
frames can see (each mistake a loader of this struct can make moves the oracle's pyramid beyond conftest.assert_close), the byte
accounting, the restatement pinned on a recorded case per format, and the host side of the entry points -- argument validation, the
refusal table, the host forms' staging of exactly the MERGED spans, and the walk loader's address function enumerated over whole
launches -- as a stand-alone program (tests/rgb_yuv_host_main.cpp) built with the library's host side under ASan + UBSan and run as a
child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
import rgb_yuv_frames as yf
import silent_oracle as so
from conftest import ROOT, assert_close
from test_rgb_nv12_host import _address_plans, needs_hipcc

NAMES = ("silent_pyramid_yuv", "silent_pyramid_yuv_dev", "silent_yuv_to_rgb", "silent_yuv_to_rgb_dev")
FORMATS = ("yuv420", "yuv422", "yuv444")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFAULT = ("bt709", "limited", "bgr")


# ----------------------------------------------------------------------------- the keyword

@pytest.mark.parametrize("kwargs", [dict(rgb_frame_format="yuv"), dict(rgb_frame_format="yuv411"), dict(rgb_frame_format="YUV420"),
                                    dict(rgb_frame_format="yuv420", mode="gray"),
                                    dict(rgb_frame_format="yuv422", rgb_frame_dtype="uint8"),
                                    dict(rgb_frame_format="yuv444", rgb_frame_dtype="uint8", rgb_frame_layout="strided"),
                                    dict(rgb_frame_format="yuv420", hw=(63, 96)), dict(rgb_frame_format="yuv420", hw=(64, 97)),
                                    dict(rgb_frame_format="yuv422", hw=(64, 97))])
def test_pipeline_refuses_bad_rgb_frame_format_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("mode", "rgb")
    hw = kwargs.pop("hw", (64, 96))
    with pytest.raises(ValueError, match="rgb_frame_format"):
        LineEndPipeline(hw, batch=1, **kwargs)


@pytest.mark.parametrize("fmt", FORMATS)
def test_bt2020_stays_for_the_deeper_formats(fmt):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match="nv12_matrix must be 'bt601', 'bt709' or"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_format=fmt, nv12_matrix="bt2020")


def test_check_rgb_frame_format():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_format
    assert tuple(_runtime.YUV_SHIFTS) == FORMATS and _runtime.YUV_SHIFTS == {"yuv420": (1, 1), "yuv422": (1, 0), "yuv444": (0, 0)}
    for fmt in FORMATS:
        assert chk(fmt) == fmt and chk(fmt, "rgb", hw=(24, 34)) == fmt
        name = "rgb_frame_format='%s' " % fmt
        for args, text in (((fmt, "gray"), r"is for mode 'rgb' \(mode 'gray' reads the luma plane through frame_layout='strided'\)"),
                           ((fmt, "rgb", "uint8"), "does not combine with rgb_frame_dtype='uint8'"),
                           ((fmt, "rgb", "float32", "strided"), "does not combine with rgb_frame_layout='strided'"),
                           ((fmt, "rgb", "float32", "packed", "uint8"), "does not combine with frame_dtype='uint8'"),
                           ((fmt, "rgb", "float32", "packed", "float32", 3), "does not combine with frame_channels=3"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "strided"), "does not combine with frame_layout='strided'")):
            with pytest.raises(ValueError, match=name + text):
                chk(*args)
        # the order: mode, combinations, extents
        with pytest.raises(ValueError, match="is for mode 'rgb'"):
            chk(fmt, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))
        with pytest.raises(ValueError, match="rgb_frame_dtype='uint8'"):
            chk(fmt, "rgb", "uint8", "strided", "uint8", 3, "strided", (3, 5))
        with pytest.raises(ValueError, match="rgb_frame_layout='strided'"):
            chk(fmt, "rgb", "float32", "strided", "uint8", 3, "strided", (3, 5))
    # extents: 4:2:0 needs even H and W, 4:2:2 even W, 4:4:4 nothing
    ok = ("rgb", "float32", "packed", "float32", 1, "packed")
    for hw in ((25, 34), (24, 33)):
        with pytest.raises(ValueError, match=r"rgb_frame_format='yuv420' needs even H and W \(4:2:0 chroma\)"):
            chk("yuv420", *ok, hw)
    with pytest.raises(ValueError, match=r"rgb_frame_format='yuv422' needs even W \(4:2:2 chroma\)"):
        chk("yuv422", *ok, (24, 33))
    assert chk("yuv422", *ok, (25, 34)) == "yuv422" and chk("yuv444", *ok, (25, 33)) == "yuv444"
    # the name first; the bare "yuv" stays a bad name; the message keeps its beginning and appends the new names
    for bad in ("yuv", "yuv440", None, 3, "Yuv420"):
        with pytest.raises(ValueError, match=r"must be 'interleaved' or 'nv12', or 'p010' / 'p012' / 'p016', or 'yuv420' / 'yuv422' / 'yuv444', got"):
            chk(bad, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))


def test_no_new_keyword():
    import inspect
    from pysilent_amd.pipeline import LineEndPipeline
    names = list(inspect.signature(LineEndPipeline.__init__).parameters)
    assert names[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"]
    from pysilent_amd._runtime import PyramidPlan
    assert list(inspect.signature(PyramidPlan.run).parameters)[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"]


# ----------------------------------------------------------------------------- yuv_frames_of, yuv_planes

N, H, W = 2, 24, 34


@pytest.mark.parametrize("name", yf.PYTHON_LAYOUTS)
def test_yuv_frames_of_on_every_layout(name):
    """The triple passes as it is: the struct's fields are the views' addresses and strides, nothing is converted or copied."""
    from pysilent_amd._runtime import yuv_frames_of
    s = yf.spec(name, N, H, W)
    Y, U, V = yf.batch(s)
    m, oy = nf.coefficients(*DEFAULT)
    for fill in yf.FILLS:
        parents = yf.place(s, Y, U, V, fill)
        y, u, v = yf.views(s, parents)
        assert np.array_equal(y, Y) and np.array_equal(u, U) and np.array_equal(v, V)
        masks = yf.pixel_mask(s)
        assert all(np.all(p[~k] == fill) for p, k in zip(parents, masks))
        assert sum(int(k.sum()) for k in masks) == N * H * W + 2 * N * (H >> s["sy"]) * (W >> s["sx"])
        args, n, dev = yuv_frames_of((y, u, v), (H, W), s["fmt"], m, oy)
        want = yf.struct_args(s, [p.ctypes.data for p in parents], m, oy)
        assert args[:11] == want[:11] and n == N and not dev, (args[:11], want[:11])
        assert np.array_equal(np.array(args[11], np.float32), m.reshape(9)) and args[12] == 16.0
        assert all(np.shares_memory(a, parents[s[p][0]]) for a, p in zip((y, u, v), "yuv"))


def test_yuv_frames_of_refusals():
    from pysilent_amd._runtime import yuv_frames_of
    s = yf.spec("i420", N, H, W)
    m, oy = nf.coefficients(*DEFAULT)
    y, u, v = yf.views(s, yf.place(s, *yf.batch(s), 0))
    for bad, text in (((y, u), "triple"), (y, "triple"), ((y.astype(np.float32), u, v), "uint8"), ((y, u, v.astype(np.int8)), "uint8"),
                      ((y, u[:1], v), "chroma planes"), ((y, u, v[:, :, :5]), "chroma planes"), ((y[:, :23], u, v), "luma plane"),
                      ((y, u, np.ascontiguousarray(v)), "u and v must have equal strides"),
                      ((y[:, :, ::-1], u, v), "not positive"), ((y, u[:, ::-1], v[:, ::-1]), "not positive"),
                      ((np.broadcast_to(y[:1], y.shape), u, v), "overlap")):
        with pytest.raises(ValueError, match=text):
            yuv_frames_of(bad, (H, W), "yuv420", m, oy)
    with pytest.raises(ValueError, match="chroma planes"):
        yuv_frames_of((y, u, v), (H, W), "yuv444", m, oy)
    with pytest.raises(ValueError, match="fmt must be"):
        yuv_frames_of((y, u, v), (H, W), "yuv", m, oy)
    with pytest.raises(TypeError):
        yuv_frames_of((y, u, [1, 2]), (H, W), "yuv420", m, oy)


def test_a_packed_buffer_is_a_valid_triple_of_slices():
    """The issue's example: yuyv[:, :, 0::2], yuyv[:, :, 1::4], yuyv[:, :, 3::4]."""
    from pysilent_amd._runtime import yuv_frames_of
    yuyv = np.random.default_rng(2).integers(0, 256, (N, H, 2 * W)).astype(np.uint8)
    m, oy = nf.coefficients(*DEFAULT)
    args, n, _ = yuv_frames_of((yuyv[:, :, 0::2], yuyv[:, :, 1::4], yuyv[:, :, 3::4]), (H, W), "yuv422", m, oy)
    a = yuyv.ctypes.data
    assert args[:11] == (a, a + 1, a + 3, 2, 2 * W, H * 2 * W, 4, 2 * W, H * 2 * W, 1, 0) and n == N


LAYOUT_ROWS = {"i420": 3 * H // 2, "yv12": 3 * H // 2, "i422": 2 * H, "i444": 3 * H, "nv12": 3 * H // 2, "nv21": 3 * H // 2, "nv16": 2 * H,
               "yuyv": H, "uyvy": H}


@pytest.mark.parametrize("layout", sorted(LAYOUT_ROWS))
def test_yuv_planes_cuts_the_triple_out_of_surfaces(layout):
    """Every byte of the three views is the byte the layout's definition names (restated here with flat indices), nothing is copied,
    and the triple passes yuv_frames_of."""
    from pysilent_amd._runtime import yuv_frames_of
    from pysilent_amd.util.zoom import yuv_planes
    from pysilent_amd.util.zoom.yuv import YUV_LAYOUTS
    rows, pitch = LAYOUT_ROWS[layout] + 2, 80
    surf = np.random.default_rng(9).integers(0, 256, (3, rows, pitch)).astype(np.uint8)
    y, u, v = yuv_planes(surf, H, W, layout)
    fmt = YUV_LAYOUTS[layout][0]
    sx, sy = yf.SHIFTS[fmt]
    ch, cw = H >> sy, W >> sx
    assert y.shape == (3, H, W) and u.shape == v.shape == (3, ch, cw) and all(np.shares_memory(p, surf) for p in (y, u, v))
    flat = surf.reshape(3, -1)
    r, c = np.arange(ch)[:, None], np.arange(cw)[None, :]
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    if layout in ("yuyv", "uyvy"):
        yo, uo, vo = (0, 1, 3) if layout == "yuyv" else (1, 0, 2)
        want = flat[:, yy * pitch + 2 * xx + yo], flat[:, r * pitch + 4 * c + uo], flat[:, r * pitch + 4 * c + vo]
    elif layout in ("nv12", "nv21", "nv16"):
        first, second = flat[:, (H + r) * pitch + 2 * c], flat[:, (H + r) * pitch + 2 * c + 1]
        want = (flat[:, yy * pitch + xx],) + ((second, first) if layout == "nv21" else (first, second))
    else:
        cp = pitch if layout == "i444" else pitch // 2
        first, second = flat[:, H * pitch + r * cp + c], flat[:, H * pitch + ch * cp + r * cp + c]
        want = (flat[:, yy * pitch + xx],) + ((second, first) if layout == "yv12" else (first, second))
    for got, w in zip((y, u, v), want):
        assert np.array_equal(got, w)
    m, oy = nf.coefficients(*DEFAULT)
    args, n, _ = yuv_frames_of((y, u, v), (H, W), fmt, m, oy)
    assert n == 3 and args[9:11] == (sx, sy) and args[0] == surf.ctypes.data + (1 if layout == "uyvy" else 0)
    # bad extents
    for bad in (dict(H=H + 4), dict(W=pitch + 2 if layout not in ("yuyv", "uyvy") else pitch // 2 + 2), dict(W=W + 1) if sx else dict(H=0),
                dict(layout="yuv"), dict(surfaces=surf[0]), dict(surfaces=surf.astype(np.uint16))):
        with pytest.raises(ValueError, match="yuv_planes"):
            yuv_planes(**dict(dict(surfaces=surf, H=H, W=W, layout=layout), **bad))


# ----------------------------------------------------------------------------- the ABI

def test_yuv_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert "const silent_yuv_frames* frames" in " ".join(src[src.index("int " + name + "("):].split(";")[0].split()), name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["silent_pyramid_yuv"] == [vp, vp, _lib._yp, i, vp]
    assert _lib._SIGNATURES["silent_pyramid_yuv_dev"] == _lib._SIGNATURES["silent_pyramid_yuv"] + [vp]
    assert _lib._SIGNATURES["silent_yuv_to_rgb"] == [vp, _lib._yp, i, i, i, vp]
    assert _lib._SIGNATURES["silent_yuv_to_rgb_dev"] == _lib._SIGNATURES["silent_yuv_to_rgb"] + [vp]
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src


def test_library_exports_the_yuv_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


@needs_hipcc
def test_the_ctypes_struct_matches_the_c_compilers_layout():
    """sizeof(silent_yuv_frames) and the offset of every field as the host program prints them (--sizeof) against the ctypes mirror."""
    from pysilent_amd import _lib
    from test_gray_uint8_host import run_driver
    line = run_driver("rgb_yuv", "--sizeof").strip().split(" | ")
    S = _lib.YuvFrames
    assert line[0] == "sizeof %d" % ctypes.sizeof(S) and ctypes.sizeof(S) == 120
    tokens = line[1].split()
    assert tokens[0::2] == [f[0] for f in S._fields_]
    assert [int(t) for t in tokens[1::2]] == [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 116]
    p = _lib.yuv_ptr((1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 0, list(range(9)), 16.0)).contents
    assert (p.y, p.u, p.v, p.y_pixel_stride, p.y_row_stride, p.y_frame_stride, p.c_pixel_stride, p.c_row_stride, p.c_frame_stride,
            p.chroma_shift_x, p.chroma_shift_y, list(p.m), p.oy) == (1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 0, list(range(9)), 16.0)
    assert _lib.yuv_ptr(None) is None


# ----------------------------------------------------------------------------- the accounting

@pytest.mark.parametrize("fmt,per_pixel", [("yuv420", 1.5), ("yuv422", 2.0), ("yuv444", 3.0)])
def test_launch_summary_and_byte_accounting(fmt, per_pixel):
    """1 + 2 / 2^(sx + sy) bytes per pixel; over the three channels 0.5, 2 / 3 and 1.0; everything else is the float32 pipeline's."""
    from test_rgb_uint8_host import _accounting_pipeline
    h, w = 1080, 1920
    f32, p = _accounting_pipeline((h, w), "float32", 6), _accounting_pipeline((h, w), "float32", 6)
    p.rgb_frame_format = fmt
    assert "%s read in place" % fmt.upper() in p.launch_summary() and p.launch_summary().startswith(f32.launch_summary())
    assert "%.1f bytes per pixel" % per_pixel in p.launch_summary()
    assert p._frame_bytes * 3 == per_pixel and abs(float(p._frame_bytes) - {1.5: 0.5, 2.0: 2 / 3, 3.0: 1.0}[per_pixel]) < 1e-15
    frame = int(per_pixel * h * w)
    assert p.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 12 * h * w + frame
    assert p.pyramid_bytes_per_frame() == f32.pyramid_bytes_per_frame() - 12 * h * w + frame
    assert p.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    assert type(p.algorithmic_bytes_per_frame()) is int and type(p.pyramid_bytes_per_frame()) is int
    assert p.dominant_kernel_name() == f32.dominant_kernel_name()


# ----------------------------------------------------------------------------- the restatement, pinned

PINNED = {"yuv420": "i420", "yuv422": "yuyv", "yuv444": "vuya"}


def test_the_restatement_is_pinned_on_a_recorded_case_per_format():
    """SHA-256 of truth() -- NumPy gather with >> sx, >> sy + convert_yuv -- on one fixed 2 x 24 x 34 batch per format (I420, YUYV,
    VUYA; bt709 / limited / bgr), the same under both fills."""
    recorded = dict(l.rsplit(" ", 1) for l in open(os.path.join(GOLDEN, "yuv_convert_sha256.txt")).read().strip().split("\n"))
    assert sorted(recorded) == sorted(PINNED)
    m, oy = nf.coefficients(*DEFAULT)
    for fmt, name in PINNED.items():
        s = yf.spec(name, N, H, W)
        assert s["fmt"] == fmt
        Y, U, V = yf.batch(s, seed=1)
        outs = [yf.truth(s, yf.place(s, Y, U, V, fill), m, oy) for fill in yf.FILLS]
        assert outs[0].dtype == np.float32 and outs[0].shape == (N, H, W, 3) and np.array_equal(outs[0], outs[1])
        assert nf.digest(outs[0]) == recorded[fmt], fmt
        assert np.any(outs[0] != np.round(outs[0])) and np.any(outs[0] == 0) and np.any(outs[0] == 255)


def test_a_420_triple_restates_the_nv12_oracle():
    """The "nv12" layout is the surfaces of tests/rgb_nv12_frames.py: the two oracles agree on them."""
    s = yf.spec("nv12", N, H, W)
    y, uv = nf.batch(N, H, W, seed=3)
    m, oy = nf.coefficients(*DEFAULT)
    py, pu = nf.place(y, uv, 0xFF)
    assert np.array_equal(yf.truth(s, [py, pu], m, oy), nf.convert(y, uv, m, oy))
    vy, vu, vv = yf.views(s, [py, pu])
    assert np.array_equal(vu, uv[..., 0]) and np.array_equal(vv, uv[..., 1]) and vv.ctypes.data == vu.ctypes.data + 1


# ----------------------------------------------------------------------------- what the frames can see

def _beyond_assert_close(got, want, what):
    """True when conftest.assert_close, with the rounding bound of the zoom, refuses ``got`` for ``want`` on some level."""
    for l, (g, w) in enumerate(zip(got, want)):
        try:
            assert_close(g.astype(np.float32), w, 1e-5, scale=255.0, what="%s level %d" % (what, l), bound=eb.zoom(w))
        except AssertionError:
            return True
    return False


@pytest.fixture(scope="module")
def correct():
    """Per layout: (spec, batch, coefficients, the true frames, their oracle pyramids), computed once."""
    out = {}
    m, oy = nf.coefficients(*DEFAULT)
    for name in yf.LAYOUTS:
        s = yf.spec(name, N, H, W)
        Y, U, V = yf.batch(s)
        frames = yf.truth(s, yf.place(s, Y, U, V, 0), m, oy)
        out[name] = (s, (Y, U, V), (m, oy), frames, [so.classic_pyramid(f, 2.0, 2) for f in frames])
    return out


@pytest.mark.parametrize("name", list(yf.LAYOUTS))
def test_the_parents_carry_the_batch_under_both_fills(correct, name):
    s, (Y, U, V), (m, oy), frames, want = correct[name]
    yy, xx = np.arange(H)[:, None] >> s["sy"], np.arange(W)[None, :] >> s["sx"]
    assert np.array_equal(frames, nf.convert_yuv(Y, U[:, yy, xx], V[:, yy, xx], m, oy))
    for fill in yf.FILLS:
        parents = yf.place(s, Y, U, V, fill)
        seen = yf.see(s, parents, m, oy)
        assert np.array_equal(seen.view(np.uint32), frames.view(np.uint32))
        assert not _beyond_assert_close(so.classic_pyramid(seen[1], 2.0, 2), want[1], "truth")


def test_the_i420_layout_is_as_awkward_as_asked():
    s = yf.spec("i420", N, H, W)
    (yfr, yr, _), (cf, cr, _) = s["y"][2], s["u"][2]
    assert cr != yr // 2 and 2 * cr != yr and yfr != H * yr and cf != (H // 2) * cr and all(s[p][1] % 2 == 1 for p in "yuv")
    for name in ("yuyv", "uyvy"):
        assert yf.spec(name, N, H, W)["y"][2][1] > 2 * W


MISTAKE_CASES = [(l, k) for l in yf.LAYOUTS for k in yf.MISTAKES if yf.MISTAKES[k][0](yf.spec(l, N, H, W))]


def test_every_mistake_has_a_layout_that_shows_it():
    assert {k for _, k in MISTAKE_CASES} == set(yf.MISTAKES)
    assert {l for l, _ in MISTAKE_CASES} == set(yf.LAYOUTS)


@pytest.mark.parametrize("layout,name", MISTAKE_CASES, ids=["%s-%s" % (l, k.replace(" ", "_")) for l, k in MISTAKE_CASES])
def test_the_parents_separate_each_mistake_from_the_truth(correct, layout, name):
    """The oracle's pyramid of what a mistaken loader would see differs from the true one by more than assert_close allows, under at
    least one of the two fills, on every frame where the mistake acts (frame 1 alone for a frame stride)."""
    s, (Y, U, V), (m, oy), frames, want = correct[layout]
    hit = (1,) if "frame stride" in name else (0, 1)
    shown = False
    for fill in yf.FILLS:
        seen = yf.see(s, yf.place(s, Y, U, V, fill), m, oy, **yf.MISTAKES[name][1](s))
        assert seen.shape == frames.shape and seen.dtype == np.float32
        shown = shown or all(_beyond_assert_close(so.classic_pyramid(seen[f], 2.0, 2), want[f], name) for f in hit)
    assert shown, "%s is invisible on the %s parents" % (name, layout)


# ----------------------------------------------------------------------------- the host side under the sanitizers

@needs_hipcc
def test_yuv_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Both forms of both entry points, for a classic and a crop plan, on I420 planes that are three heap blocks of exactly their
    spans, a YUYV buffer that is ONE heap block of exactly the union of its spans and NV12 surfaces as a triple: the host forms stage
    the merged intervals -- three, ONE (the YUYV buffer is copied once) and two -- byte for byte, and the poisoned arena behind each
    is untouched; a byte one past a span is never read (AddressSanitizer would report it); status codes and the order of the checks.
    No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb yuv host main ok" in run_driver("rgb_yuv")


@needs_hipcc
def test_every_single_fault_of_the_yuv_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb_yuv", "--refusals").strip().split("\n")
    want = open(os.path.join(GOLDEN, "yuv_refusals.txt")).read().strip().split("\n")
    assert len(want) == 2 * 23 + 2 * 20 and {l.split(" | ")[0] for l in want} == set(NAMES)
    assert got == want
    for l in want:
        name, case, status, text = l.split(" | ")
        assert text.startswith(name.replace("_dev", "") + ": "), l
        assert status == ("-4" if case == "single-channel plan" else "-1"), l
    single = [l for l in want if "single-channel plan" in l]
    assert len(single) == 2 and all("silent_pyramid_view)" in l for l in single)
    assert sum("chroma shift must be 0 or 1" in l for l in want) == 8 and sum("must be finite" in l for l in want) == 8
    assert sum("even extent" in l for l in want) == 8 and sum("pixel stride is below 1" in l for l in want) == 8


ADDRESS_LAYOUTS = ("i420", "yuyv", "nv21", "i422", "vuya", "yuv440")
ADDRESS_CASES = [(l, w) for l in ADDRESS_LAYOUTS for w in range(4) if l in ("i420", "yuyv") or w in (1, 3)]


@needs_hipcc
@pytest.mark.parametrize("layout,which", ADDRESS_CASES, ids=["%s-%s" % (l, ("classic-40x8", "classic-64x66", "classic-134x242", "crops-270x482")[w])
                                                             for l, w in ADDRESS_CASES])
def test_every_address_of_the_walk_loader_is_a_pixels_byte_and_the_crops_are_covered(layout, which):
    """--addresses: w3_yuv_load -- the function pyramid_walk3_kernel forms its YUV loads with -- for every block, chunk, row, lane and
    load slot of the plan's launch on two frames: every offset is that of a byte that is some pixel's Y, U or V of its plane (so
    nothing between the pixels of a packed buffer and nothing outside a span), and the Y, U and V byte of every crop pixel is among
    the bytes touched."""
    from test_gray_uint8_host import run_driver
    hw, levels = _address_plans()[which]
    out = run_driver("rgb_yuv", "--addresses", layout, str(hw[0]), str(hw[1]), str(len(levels)), *[str(int(v)) for l in levels for v in l])
    lines = [l for l in out.strip().split("\n") if l]
    assert len(lines) == 1, out
    f = lines[0].split(" | ")
    assert f[0] == "%s %d x %d" % ((layout,) + hw) and f[3] == "outside 0" and f[4].endswith("missing y 0 u 0 v 0") and f[5] == "not a pixel byte 0", lines[0]
    assert int(f[4].split()[1]) > 0 and int(f[2].split()[1]) > 0, lines[0]
    if which == 3:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
        assert "plans 2 " in f[1] and int(f[6].split()[2]) >= 1, lines[0]
