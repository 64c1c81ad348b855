"""16-bit planar, semi-planar and packed YUV for 3-channel plans (rgb_frame_format="yuv420p10" ... "yuv444p16", silent_pyramid_yuv16[_dev],
silent_yuv16_to_rgb[_dev]) without a GPU: the keyword's refusals and their order (before any torch or GPU work), yuv16_frames_of and
yuv16_planes on every layout, the symbols and the struct (its ctypes mirror against the C compiler's sizeof / offsets), the
restatement of the conversion pinned by SHA-256 and checked against the P010 and 8-bit YUV restatements, what the test frames can see
(each mistake a loader of this struct can make moves the oracle's pyramid beyond conftest.assert_close), the byte accounting, and the
host side of the entry points -- argument validation, the refusal table, the host forms' staging of exactly the MERGED spans, and the
walk loader's address function enumerated over whole launches -- as a stand-alone program (tests/rgb_yuv16_host_main.cpp) built with
the library's host side under ASan + UBSan and run as a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
import rgb_p010_frames as pf
import rgb_yuv16_frames as wf
import silent_oracle as so
from conftest import ROOT, assert_close
from test_rgb_nv12_host import _address_plans, needs_hipcc

NAMES = ("silent_pyramid_yuv16", "silent_pyramid_yuv16_dev", "silent_yuv16_to_rgb", "silent_yuv16_to_rgb_dev")
FORMATS = tuple("yuv%sp%s" % (x, d) for x in ("420", "422", "444") for d in ("10", "12", "10msb", "12msb", "16"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N, H, W = 2, 24, 34


# ----------------------------------------------------------------------------- the keyword

def test_the_fifteen_names():
    from pysilent_amd import _runtime
    assert sorted(_runtime.YUV16_FORMATS) == sorted(FORMATS) and len(FORMATS) == 15
    for x, (sx, sy) in (("420", (1, 1)), ("422", (1, 0)), ("444", (0, 0))):
        assert _runtime.YUV16_FORMATS["yuv%sp10" % x] == (sx, sy, 10, 0) and _runtime.YUV16_FORMATS["yuv%sp12" % x] == (sx, sy, 12, 0)
        assert _runtime.YUV16_FORMATS["yuv%sp10msb" % x] == (sx, sy, 10, 6) and _runtime.YUV16_FORMATS["yuv%sp12msb" % x] == (sx, sy, 12, 4)
        assert _runtime.YUV16_FORMATS["yuv%sp16" % x] == (sx, sy, 16, 0)
    # the 8-bit family and P010 keep their tables
    assert tuple(_runtime.YUV_SHIFTS) == ("yuv420", "yuv422", "yuv444") and _runtime.P010_DEPTHS == {"p010": 10, "p012": 12, "p016": 16}


@pytest.mark.parametrize("kwargs", [dict(rgb_frame_format="yuv420p"), dict(rgb_frame_format="yuv420p8"), dict(rgb_frame_format="yuv420p10le"),
                                    dict(rgb_frame_format="yuv440p10"), dict(rgb_frame_format="yuv420p16msb"), dict(rgb_frame_format="YUV420P10"),
                                    dict(rgb_frame_format="yuv420p10", mode="gray"),
                                    dict(rgb_frame_format="yuv422p12", rgb_frame_dtype="uint8"),
                                    dict(rgb_frame_format="yuv444p16", rgb_frame_dtype="uint8", rgb_frame_layout="strided"),
                                    dict(rgb_frame_format="yuv420p10msb", hw=(63, 96)), dict(rgb_frame_format="yuv420p12", hw=(64, 97)),
                                    dict(rgb_frame_format="yuv422p10", hw=(64, 97))])
def test_pipeline_refuses_bad_rgb_frame_format_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("mode", "rgb")
    hw = kwargs.pop("hw", (64, 96))
    with pytest.raises(ValueError, match="rgb_frame_format"):
        LineEndPipeline(hw, batch=1, **kwargs)


@pytest.mark.parametrize("fmt", FORMATS)
def test_bt2020_is_accepted_and_the_coefficients_are_p010s(fmt):
    from pysilent_amd import _runtime
    depth = _runtime.YUV16_FORMATS[fmt][2]
    m, oy, oc = _runtime.p010_coefficients("bt2020", "limited", "rgb", depth)
    wm, woy, woc = pf.coefficients("bt2020", "limited", "rgb", depth)
    assert np.array_equal(m, wm) and oy == woy and oc == woc
    with pytest.raises(ValueError, match="nv12_matrix must be 'bt601', 'bt709', 'bt2020' or"):
        _runtime.p010_coefficients("bt2100", "limited", "rgb", depth)


def test_check_rgb_frame_format():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_format
    for fmt in FORMATS:
        assert chk(fmt) == fmt and chk(fmt, "rgb", hw=(24, 34)) == fmt
        name = "rgb_frame_format='%s' " % fmt
        for args, text in (((fmt, "gray"), r"is for mode 'rgb' \(mode 'gray' reads the luma plane through frame_layout='strided' with frame_dtype='uint16'\)"),
                           ((fmt, "rgb", "uint8"), r"does not combine with rgb_frame_dtype='uint8' \(the planes are uint16"),
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
    ok = ("rgb", "float32", "packed", "float32", 1, "packed")
    for hw in ((25, 34), (24, 33)):
        with pytest.raises(ValueError, match=r"rgb_frame_format='yuv420p10' needs even H and W \(4:2:0 chroma\)"):
            chk("yuv420p10", *ok, hw)
    with pytest.raises(ValueError, match=r"rgb_frame_format='yuv422p10msb' needs even W \(4:2:2 chroma\)"):
        chk("yuv422p10msb", *ok, (24, 33))
    assert chk("yuv422p16", *ok, (25, 34)) == "yuv422p16" and chk("yuv444p12", *ok, (25, 33)) == "yuv444p12"
    # the name first; the message keeps its beginning and names the new family
    for bad in ("yuv420p", "yuv420p14", None, 3, "yuv440p10"):
        with pytest.raises(ValueError, match=r"must be 'interleaved' or 'nv12', or 'p010' / 'p012' / 'p016', or 'yuv420' / 'yuv422' / 'yuv444', got .*"
                                             r"'yuvXp10' / 'yuvXp12' / 'yuvXp10msb' / 'yuvXp12msb' / 'yuvXp16'"):
            chk(bad, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))
    # every previously valid or refused value behaves as before
    for fmt in ("interleaved", "nv12", "p010", "p012", "p016", "yuv420", "yuv422", "yuv444"):
        assert chk(fmt) == fmt
    with pytest.raises(ValueError, match=r"mode 'gray' reads the luma plane through frame_layout='strided'\)"):
        chk("nv12", "gray")
    with pytest.raises(ValueError, match=r"frame_layout='strided' with frame_dtype='uint16'\)"):
        chk("p010", "gray")
    with pytest.raises(ValueError, match="rgb_frame_format='p010' needs even H and W"):
        chk("p010", *ok, (25, 34))


def test_no_new_keyword():
    import inspect
    from pysilent_amd.pipeline import LineEndPipeline
    names = list(inspect.signature(LineEndPipeline.__init__).parameters)
    assert names[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"] and len(names) == 36
    from pysilent_amd._runtime import PyramidPlan
    assert list(inspect.signature(PyramidPlan.run).parameters)[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"]


# ----------------------------------------------------------------------------- yuv16_frames_of, yuv16_planes

@pytest.mark.parametrize("name", wf.PYTHON_LAYOUTS)
def test_yuv16_frames_of_on_every_layout(name):
    """The triple passes as it is, as NumPy views and as torch CPU tensors: the struct's fields are the views' addresses and BYTE
    strides, nothing is converted or copied."""
    import torch
    from pysilent_amd._runtime import yuv16_frames_of
    s = wf.spec(name, N, H, W)
    Y, U, V = wf.batch(s)
    m, oy, oc = wf.coefficients(depth=s["depth"])
    for fill in wf.FILLS:
        parents = wf.place(s, Y, U, V, fill)
        y, u, v = wf.views(s, parents)
        assert np.array_equal(y, Y) and np.array_equal(u, U) and np.array_equal(v, V)
        masks = wf.pixel_mask(s)
        assert all(np.all(p[~k] == fill * 0x0101) for p, k in zip(parents, masks))
        assert sum(int(k.sum()) for k in masks) == N * H * W + 2 * N * (H >> s["sy"]) * (W >> s["sx"])
        args, n, dev = yuv16_frames_of((y, u, v), (H, W), s["fmt"], m, oy, oc)
        want = wf.struct_args(s, [p.ctypes.data for p in parents], m, oy, oc)
        assert args[:11] == want[:11] and args[13:] == want[13:] and n == N and not dev, (args[:11], want[:11])
        assert np.array_equal(np.array(args[11], np.float32), m.reshape(9)) and args[12] == float(oy)
        assert all(a % 2 == 0 for a in args[:9])
        tp = [torch.from_numpy(p) for p in parents]
        targs, tn, tdev = yuv16_frames_of(wf.torch_views(s, tp), (H, W), s["fmt"], m, oy, oc)
        assert targs[:11] == want[:11] and tn == N and not tdev


def test_the_awkward_geometry_that_was_asked_for():
    s = wf.spec("i010", N, H, W)
    (yf, yr, _), (cf, cr, _) = s["y"][2], s["u"][2]
    assert (2 * yr) % 4 == 2 and (2 * cr) % 4 == 2                           # row strides no multiple of 4 bytes
    assert all(s[p][1] % 2 == 1 for p in "yuv")                              # plane addresses 2 (mod 4) in 4-byte aligned parents
    assert cr != yr // 2 and 2 * cr != yr and yf != H * yr and cf != (H // 2) * cr
    assert wf.spec("y210", N, H, W)["y"][2][1] > 2 * W and wf.spec("p010", N, H, W)["v"][1] == wf.spec("p010", N, H, W)["u"][1] + 1


def test_yuv16_frames_of_refusals():
    from pysilent_amd._runtime import yuv16_frames_of
    s = wf.spec("i010", N, H, W)
    m, oy, oc = wf.coefficients()
    parents = wf.place(s, *wf.batch(s), 0)
    y, u, v = wf.views(s, parents)
    st = np.lib.stride_tricks.as_strided
    odd_rows = st(parents[0].view(np.uint8)[6:].view(np.uint16), y.shape, (y.strides[0], y.strides[1] + 1, 2))
    for bad, text in (((y, u), "triple"), (y, "triple"), ((y.astype(np.float32), u, v), "uint16"), ((y, u, v.astype(np.int16)), "uint16"),
                      ((y.astype(np.uint8), u, v), "uint16"),
                      ((y, u[:1], v), "chroma planes"), ((y, u, v[:, :, :5]), "chroma planes"), ((y[:, :23], u, v), "luma plane"),
                      ((y, u, np.ascontiguousarray(v)), "u and v must have equal strides"),
                      ((y[:, :, ::-1], u, v), "not positive"), ((y, u[:, ::-1], v[:, ::-1]), "not positive"),
                      ((np.broadcast_to(y[:1], y.shape), u, v), "overlap"),
                      ((odd_rows, u, v), "odd")):
        with pytest.raises(ValueError, match=text):
            yuv16_frames_of(bad, (H, W), "yuv420p10", m, oy, oc)
    with pytest.raises(ValueError, match="chroma planes"):
        yuv16_frames_of((y, u, v), (H, W), "yuv444p10", m, oy, oc)
    with pytest.raises(ValueError, match="fmt must be"):
        yuv16_frames_of((y, u, v), (H, W), "yuv420", m, oy, oc)
    with pytest.raises(TypeError):
        yuv16_frames_of((y, u, [1, 2]), (H, W), "yuv420p10", m, oy, oc)


def test_a_y210_buffer_is_a_valid_triple_of_slices():
    from pysilent_amd._runtime import yuv16_frames_of
    y210 = np.random.default_rng(2).integers(0, 1 << 16, (N, H, 2 * W)).astype(np.uint16)
    m, oy, oc = wf.coefficients()
    args, n, _ = yuv16_frames_of((y210[:, :, 0::2], y210[:, :, 1::4], y210[:, :, 3::4]), (H, W), "yuv422p10msb", m, oy, oc)
    a = y210.ctypes.data
    assert args[:11] == (a, a + 2, a + 6, 4, 4 * W, H * 4 * W, 8, 4 * W, H * 4 * W, 1, 0) and n == N and args[14:] == (6, 10)


LAYOUT_ROWS = {"i010": 3 * H // 2, "i012": 3 * H // 2, "i210": 2 * H, "i212": 2 * H, "i410": 3 * H, "i412": 3 * H,
               "p010": 3 * H // 2, "p012": 3 * H // 2, "p016": 3 * H // 2, "p210": 2 * H, "p216": 2 * H, "p410": 2 * H, "p416": 2 * H,
               "y210": H, "y212": H, "y216": H}


@pytest.mark.parametrize("tensors", ["numpy", "torch"])
@pytest.mark.parametrize("layout", sorted(LAYOUT_ROWS))
def test_yuv16_planes_cuts_the_triple_out_of_surfaces(layout, tensors):
    """Every element of the three views is the element the layout's definition names (restated here with flat indices), nothing is
    copied, and the triple passes yuv16_frames_of with the format's depth and shift."""
    import torch
    from pysilent_amd import _runtime
    from pysilent_amd.util.zoom import yuv16_planes, YUV16_LAYOUTS
    assert sorted(YUV16_LAYOUTS) == sorted(LAYOUT_ROWS)
    rows, pitch = LAYOUT_ROWS[layout] + 2, 80
    surf = np.random.default_rng(9).integers(0, 1 << 16, (3, rows, pitch)).astype(np.uint16)
    fmt = YUV16_LAYOUTS[layout]
    sx, sy, depth, shift = _runtime.YUV16_FORMATS[fmt]
    assert depth == {"0": 10, "2": 12, "6": 16}[layout[3]] and shift == (0 if layout[0] == "i" else 16 - depth)
    assert (sx, sy) == {"0": (1, 1), "2": (1, 0), "4": (0, 0)}[layout[1]] if layout[0] != "y" else (sx, sy) == (1, 0)
    planes = yuv16_planes(torch.from_numpy(surf) if tensors == "torch" else surf, H, W, layout)
    y, u, v = (p.numpy() if tensors == "torch" else p for p in planes)
    ch, cw = H >> sy, W >> sx
    assert y.shape == (3, H, W) and u.shape == v.shape == (3, ch, cw) and all(np.shares_memory(p, surf) for p in (y, u, v))
    flat = surf.reshape(3, -1)
    r, c = np.arange(ch)[:, None], np.arange(cw)[None, :]
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    if layout[0] == "y":
        want = flat[:, yy * pitch + 2 * xx], flat[:, r * pitch + 4 * c + 1], flat[:, r * pitch + 4 * c + 3]
    elif layout[0] == "p":
        want = flat[:, yy * pitch + xx], flat[:, (H + r) * pitch + 2 * c], flat[:, (H + r) * pitch + 2 * c + 1]
    else:
        cp = pitch if sx == 0 else pitch // 2
        want = flat[:, yy * pitch + xx], flat[:, H * pitch + r * cp + c], flat[:, H * pitch + ch * cp + r * cp + c]
    for got, w in zip((y, u, v), want):
        assert np.array_equal(got, w)
    m, oy, oc = wf.coefficients(depth=depth)
    args, n, _ = _runtime.yuv16_frames_of(planes, (H, W), fmt, m, oy, oc)
    assert n == 3 and args[9:11] == (sx, sy) and args[14:] == (shift, depth) and args[0] == surf.ctypes.data
    for bad in (dict(H=H + 4), dict(W=pitch + 2 if layout[0] != "y" else pitch // 2 + 2), dict(W=W + 1) if sx else dict(H=0),
                dict(layout="i420"), dict(surfaces=surf[0]), dict(surfaces=surf.astype(np.uint8)), dict(surfaces=surf.astype(np.int16))):
        with pytest.raises(ValueError, match="yuv16_planes"):
            yuv16_planes(**dict(dict(surfaces=surf, H=H, W=W, layout=layout), **bad))


# ----------------------------------------------------------------------------- the ABI

def test_yuv16_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert "const silent_yuv16_frames* frames" in " ".join(src[src.index("int " + name + "("):].split(";")[0].split()), name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["silent_pyramid_yuv16"] == [vp, vp, _lib._y16p, i, vp]
    assert _lib._SIGNATURES["silent_pyramid_yuv16_dev"] == _lib._SIGNATURES["silent_pyramid_yuv16"] + [vp]
    assert _lib._SIGNATURES["silent_yuv16_to_rgb"] == [vp, _lib._y16p, i, i, i, vp]
    assert _lib._SIGNATURES["silent_yuv16_to_rgb_dev"] == _lib._SIGNATURES["silent_yuv16_to_rgb"] + [vp]
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src


def test_library_exports_the_yuv16_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


@needs_hipcc
def test_the_ctypes_struct_matches_the_c_compilers_layout():
    """sizeof(silent_yuv16_frames) and the offset of every field as the host program prints them (--sizeof) against the ctypes mirror."""
    from pysilent_amd import _lib
    from test_gray_uint8_host import run_driver
    line = run_driver("rgb_yuv16", "--sizeof").strip().split(" | ")
    S = _lib.Yuv16Frames
    assert line[0] == "sizeof %d" % ctypes.sizeof(S) and ctypes.sizeof(S) == 136
    tokens = line[1].split()
    assert tokens[0::2] == [f[0] for f in S._fields_]
    assert [int(t) for t in tokens[1::2]] == [getattr(S, f[0]).offset for f in S._fields_] \
        == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 116, 120, 124, 128]
    p = _lib.yuv16_ptr((2, 4, 6, 4, 5, 6, 7, 8, 9, 1, 0, list(range(9)), 64.0, 512.0, 6, 10)).contents
    assert (p.y, p.u, p.v, p.y_pixel_stride, p.y_row_stride, p.y_frame_stride, p.c_pixel_stride, p.c_row_stride, p.c_frame_stride,
            p.chroma_shift_x, p.chroma_shift_y, list(p.m), p.oy, p.oc, p.shift, p.depth) \
        == (2, 4, 6, 4, 5, 6, 7, 8, 9, 1, 0, list(range(9)), 64.0, 512.0, 6, 10)
    assert _lib.yuv16_ptr(None) is None


# ----------------------------------------------------------------------------- the accounting

@pytest.mark.parametrize("fmt,per_pixel", [("yuv420p10", 3), ("yuv422p10msb", 4), ("yuv444p16", 6), ("yuv420p12msb", 3), ("yuv422p12", 4)])
def test_launch_summary_and_byte_accounting(fmt, per_pixel):
    """2 (1 + 2 / 2^(sx + sy)) bytes per pixel: 3, 4 and 6; everything else is the float32 pipeline's."""
    from test_rgb_uint8_host import _accounting_pipeline
    h, w = 1080, 1920
    f32, p = _accounting_pipeline((h, w), "float32", 6), _accounting_pipeline((h, w), "float32", 6)
    p.rgb_frame_format = fmt
    assert "%s read in place" % fmt.upper() in p.launch_summary() and p.launch_summary().startswith(f32.launch_summary())
    assert "triple of uint16 views, %d bytes per pixel" % per_pixel in p.launch_summary()
    assert p._frame_bytes * 3 == per_pixel
    frame = per_pixel * h * w
    assert p.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 12 * h * w + frame
    assert p.pyramid_bytes_per_frame() == f32.pyramid_bytes_per_frame() - 12 * h * w + frame
    assert p.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    assert type(p.algorithmic_bytes_per_frame()) is int and type(p.pyramid_bytes_per_frame()) is int
    assert p.dominant_kernel_name() == f32.dominant_kernel_name()


# ----------------------------------------------------------------------------- the restatement: pinned, and against its relatives

PINNED = {"420": "i010", "422": "y210", "444": "i410"}


def test_the_restatement_is_pinned_on_a_recorded_case_per_subsampling():
    """SHA-256 of truth() -- NumPy gather with >> sx, >> sy, shift and mask, separately rounded float32 operations -- on one fixed
    2 x 24 x 34 batch per subsampling (I010, Y210, I410; bt709 / limited / bgr), the same under both fills."""
    recorded = dict(l.rsplit(" ", 1) for l in open(os.path.join(GOLDEN, "yuv16_convert_sha256.txt")).read().strip().split("\n"))
    assert sorted(recorded) == sorted(PINNED)
    m, oy, oc = wf.coefficients()
    for sub, name in PINNED.items():
        s = wf.spec(name, N, H, W)
        assert s["sub"] == sub and s["depth"] == 10
        Y, U, V = wf.batch(s, seed=1)
        outs = [wf.truth(s, wf.place(s, Y, U, V, fill), m, oy, oc) for fill in wf.FILLS]
        assert outs[0].dtype == np.float32 and outs[0].shape == (N, H, W, 3) and np.array_equal(outs[0], outs[1])
        assert wf.digest(outs[0]) == recorded[sub], sub
        assert np.any(outs[0] != np.round(outs[0])) and np.any(outs[0] == 0) and np.any(outs[0] == 255)


@pytest.mark.parametrize("depth", pf.DEPTHS)
def test_on_a_p010_shaped_batch_it_is_the_p010_restatement(depth):
    """(a) The "p010" layout is the surfaces of tests/rgb_p010_frames.py: the two restatements agree bit for bit, for every variant."""
    y, uv = pf.batch(N, H, W, depth, seed=3)
    py, pu = pf.place(y, uv, 0xFF)
    s = dict(wf.spec("p010", N, H, W), depth=depth, shift=16 - depth)
    vy, vu, vv = wf.views(s, [py, pu])
    assert np.array_equal(vu, uv[..., 0]) and np.array_equal(vv, uv[..., 1]) and vv.ctypes.data == vu.ctypes.data + 2
    for variant in pf.VARIANTS:
        m, oy, oc = pf.coefficients(*variant, depth)
        assert np.array_equal(wf.truth(s, [py, pu], m, oy, oc).view(np.uint32), pf.convert(y, uv, m, oy, oc, 16 - depth).view(np.uint32))


@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_widened_bytes_give_the_8_bit_restatements_bits(sub):
    """(b) Limited-range coefficients are the 8-bit ones times 2^-(depth - 8) with offsets times 2^(depth - 8): low-aligned codes
    byte << (depth - 8) and high-aligned elements (byte << 8) | garbage both give the 8-bit YUV restatement's bits on the bytes."""
    sx, sy = wf.SHIFTS[sub]
    rng = np.random.default_rng(5)
    c = (N, H >> sy, W >> sx)
    B = [rng.integers(0, 256, sh).astype(np.uint8) for sh in ((N, H, W), c, c)]
    yy, xx = np.arange(H)[:, None] >> sy, np.arange(W)[None, :] >> sx
    for matrix in ("bt601", "bt709"):
        m8, oy8 = nf.coefficients(matrix, "limited", "bgr")
        want = nf.convert_yuv(B[0], B[1][:, yy, xx], B[2][:, yy, xx], m8, oy8)
        for depth in (10, 12, 16):
            m, oy, oc = wf.coefficients(matrix, "limited", "bgr", depth)
            low = [(b.astype(np.uint16) << (depth - 8)) for b in B]
            assert np.array_equal(wf.convert(*low, sx, sy, m, oy, oc, 0, depth).view(np.uint32), want.view(np.uint32)), (matrix, depth, "low")
            garbage = [((b.astype(np.uint16) << 8) | rng.integers(0, 1 << (16 - depth), b.shape).astype(np.uint16)) if depth < 16
                       else (b.astype(np.uint16) << 8) for b in B]
            assert np.array_equal(wf.convert(*garbage, sx, sy, m, oy, oc, 16 - depth, depth).view(np.uint32), want.view(np.uint32)), (matrix, depth, "high")


@pytest.mark.parametrize("name", ["i010", "i012", "y210", "m014", "i009"])
def test_bits_outside_the_code_change_nothing(name):
    """(c) The same codes with zeros, with ones and with random bits outside [shift, shift + depth)."""
    s = wf.spec(name, N, H, W)
    m, oy, oc = wf.coefficients(depth=10)
    clean = wf.batch(s, junk=False)
    junk = wf.batch(s, junk=True)
    outside = np.uint16(0xFFFF & ~(((1 << s["depth"]) - 1) << s["shift"]))
    assert outside and all(np.any(j & outside) and not np.any(c & outside) and np.array_equal(j & ~outside, c) for j, c in zip(junk, clean))
    ones = tuple(c | outside for c in clean)
    want = wf.convert(*clean, s["sx"], s["sy"], m, oy, oc, s["shift"], s["depth"])
    for other in (junk, ones):
        assert np.array_equal(wf.convert(*other, s["sx"], s["sy"], m, oy, oc, s["shift"], s["depth"]).view(np.uint32), want.view(np.uint32))


def test_p16_codes_from_0x8000_do_not_go_negative():
    """(d) Full-range identity luma: the value of code c is c * 255 / 65535, monotone through 0x8000."""
    codes = np.array([0x7FFE, 0x7FFF, 0x8000, 0x8001, 0xC000, 0xFFFE, 0xFFFF], np.uint16).reshape(1, 1, 7)
    half = np.full((1, 1, 7), 0x8000, np.uint16)
    m, oy, oc = wf.coefficients("bt709", "full", "rgb", 16)
    out = wf.convert(codes, half, half, 0, 0, m, oy, oc, 0, 16)[0, 0]
    assert np.all(np.diff(out[:, 1]) >= 0) and out[2, 1] > 127 and out[-1, 1] == 255.0 and np.all(out > 100)


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
    for name in wf.LAYOUTS:
        s = wf.spec(name, N, H, W)
        Y, U, V = wf.batch(s)
        m, oy, oc = wf.coefficients(depth=s["depth"])
        frames = wf.truth(s, wf.place(s, Y, U, V, 0), m, oy, oc)
        out[name] = (s, (Y, U, V), (m, oy, oc), frames, [so.classic_pyramid(f, 2.0, 2) for f in frames])
    return out


@pytest.mark.parametrize("name", list(wf.LAYOUTS))
def test_the_parents_carry_the_batch_under_both_fills(correct, name):
    s, (Y, U, V), (m, oy, oc), frames, want = correct[name]
    assert np.array_equal(frames, wf.convert(Y, U, V, s["sx"], s["sy"], m, oy, oc, s["shift"], s["depth"]))
    for fill in wf.FILLS:
        parents = wf.place(s, Y, U, V, fill)
        seen = wf.see(s, parents, m, oy, oc)
        assert np.array_equal(seen.view(np.uint32), frames.view(np.uint32))
        assert not _beyond_assert_close(so.classic_pyramid(seen[1], 2.0, 2), want[1], "truth")


MISTAKE_CASES = [(l, k) for l in wf.LAYOUTS for k in wf.MISTAKES if wf.MISTAKES[k][0](wf.spec(l, N, H, W))]


def test_every_mistake_has_a_layout_that_shows_it_and_every_layout_a_mistake():
    assert {k for _, k in MISTAKE_CASES} == set(wf.MISTAKES) and len(wf.MISTAKES) == 9
    assert {l for l, _ in MISTAKE_CASES} == set(wf.LAYOUTS)


@pytest.mark.parametrize("layout,name", MISTAKE_CASES, ids=["%s-%s" % (l, k.replace(" ", "_")) for l, k in MISTAKE_CASES])
def test_the_parents_separate_each_mistake_from_the_truth(correct, layout, name):
    """The oracle's pyramid of what a mistaken loader would see differs from the true one by more than assert_close allows, under at
    least one of the two fills, on every frame where the mistake acts (frame 1 alone for a frame term).  A signed load shows in a
    loader that leaves out the mask where it is redundant (shift + depth == 16): behind the mask a sign extension is cut off."""
    s, (Y, U, V), (m, oy, oc), frames, want = correct[layout]
    hit = (1,) if "frame term" in name else (0, 1)
    shown = False
    for fill in wf.FILLS:
        seen = wf.see(s, wf.place(s, Y, U, V, fill), m, oy, oc, **wf.MISTAKES[name][1](s))
        assert seen.shape == frames.shape and seen.dtype == np.float32
        shown = shown or all(_beyond_assert_close(so.classic_pyramid(seen[f], 2.0, 2), want[f], name) for f in hit)
    assert shown, "%s is invisible on the %s parents" % (name, layout)


# ----------------------------------------------------------------------------- the host side under the sanitizers

@needs_hipcc
def test_yuv16_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Both forms of both entry points, for a classic and a crop plan, on I010 planes that are three heap blocks of exactly their
    spans, a Y210 buffer that is ONE heap block of exactly the union of its spans and P010 surfaces as a triple: the host forms stage
    the merged intervals -- three, ONE (the Y210 buffer is copied once) and two -- byte for byte, and the poisoned arena behind each
    is untouched; a byte one past a span is never read (AddressSanitizer would report it); status codes and the order of the checks;
    depths 8, 9 and 14.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb yuv16 host main ok" in run_driver("rgb_yuv16")


@needs_hipcc
def test_every_single_fault_of_the_yuv16_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb_yuv16", "--refusals").strip().split("\n")
    want = open(os.path.join(GOLDEN, "yuv16_refusals.txt")).read().strip().split("\n")
    assert len(want) == 2 * 33 + 2 * 30 and {l.split(" | ")[0] for l in want} == set(NAMES)
    assert got == want
    for l in want:
        name, case, status, text = l.split(" | ")
        assert text.startswith(name.replace("_dev", "") + ": "), l
        assert status == ("-4" if case == "single-channel plan" else "-1"), l
    single = [l for l in want if "single-channel plan" in l]
    assert len(single) == 2 and all("silent_pyramid_view16)" in l for l in single)
    # the header's order, per entry point: the 8-bit struct's list, then finite, alignment, strides, depth, shift, then the shared checks
    texts = [l.split(" | ")[3].split(": ", 1)[1] for l in want if l.startswith("silent_pyramid_yuv16 |")]
    order = ["NULL pointer", "a chroma shift must be 0 or 1", "a subsampled axis needs an even extent", "a pixel stride is below 2",
             "y_row_stride is below", "c_row_stride is below", "y_frame_stride is below", "c_frame_stride is below", "y_frame_stride is below",
             "a plane spans more than 2^63 bytes", "m, oy and oc must be finite", "y, u and v must be 2-byte aligned", "a stride is odd",
             "depth must be 8 .. 16", "shift must be 0 .. 16 - depth", "NULL pointer", "plan belongs to another context", "n_frames must be >= 1",
             "16-bit YUV frames are for 3-channel plans"]
    seen = [t for i, t in enumerate(texts) if i == 0 or t != texts[i - 1]]
    assert len(seen) == len(order) and all(t.startswith(o) for t, o in zip(seen, order)), seen


ADDRESS_LAYOUTS = ("i010", "y210", "p210", "i410", "yuv440", "vu010")
ADDRESS_CASES = [(l, w) for l in ADDRESS_LAYOUTS for w in range(4) if l in ("i010", "y210") or w in (1, 3)]


@needs_hipcc
@pytest.mark.parametrize("layout,which", ADDRESS_CASES, ids=["%s-%s" % (l, ("classic-40x8", "classic-64x66", "classic-134x242", "crops-270x482")[w])
                                                             for l, w in ADDRESS_CASES])
def test_every_address_of_the_walk_loader_is_a_pixels_element_and_the_crops_are_covered(layout, which):
    """--addresses: w3_yuv16_load -- the function pyramid_walk3_kernel forms its 16-bit YUV loads with -- for every block, chunk, row,
    lane and load slot of the plan's launch on two frames: every offset is the EVEN offset of an element that is some pixel's Y, U or
    V of its plane (so nothing between the pixels of a packed buffer and nothing outside a span), and the Y, U and V element of every
    crop pixel is among the elements touched."""
    from test_gray_uint8_host import run_driver
    hw, levels = _address_plans()[which]
    out = run_driver("rgb_yuv16", "--addresses", layout, str(hw[0]), str(hw[1]), str(len(levels)), *[str(int(v)) for l in levels for v in l])
    lines = [l for l in out.strip().split("\n") if l]
    assert len(lines) == 1, out
    f = lines[0].split(" | ")
    assert f[0] == "%s %d x %d" % ((layout,) + hw) and f[3] == "outside 0" and f[4].endswith("missing y 0 u 0 v 0"), lines[0]
    assert f[5] == "not a pixel element 0" and f[7] == "odd offsets 0", lines[0]
    assert int(f[4].split()[1]) > 0 and int(f[2].split()[1]) > 0, lines[0]
    if which == 3:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
        assert "plans 2 " in f[1] and int(f[6].split()[2]) >= 1, lines[0]
