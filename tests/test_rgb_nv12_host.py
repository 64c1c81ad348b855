"""NV12 decoder surfaces for 3-channel plans (rgb_frame_format="nv12", silent_pyramid_nv12[_dev], silent_nv12_to_rgb[_dev]) without a
GPU: the keyword's refusals (before any torch or GPU work), the symbols and the struct, the coefficients against their closed forms,
the NumPy restatement of the conversion pinned on a recorded case, what the test frames can see (each mistake an NV12 loader can make
moves the oracle's pyramid beyond conftest.assert_close), the byte accounting, and the host side of the entry points -- argument
validation, the refusal table, the host forms' staging of exactly the two spans, and the walk loader's address function enumerated
over whole launches -- as a stand-alone program (tests/rgb_nv12_host_main.cpp) built with the library's host side under ASan + UBSan
and run as a child process."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
import silent_oracle as so
from conftest import ROOT, assert_close

NAMES = ("silent_pyramid_nv12", "silent_pyramid_nv12_dev", "silent_nv12_to_rgb", "silent_nv12_to_rgb_dev")
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ----------------------------------------------------------------------------- the keyword

@pytest.mark.parametrize("kwargs", [dict(rgb_frame_format="yuv"), dict(rgb_frame_format=None), dict(rgb_frame_format=12),
                                    dict(rgb_frame_format="NV12"),
                                    dict(rgb_frame_format="nv12", mode="gray"),
                                    dict(rgb_frame_format="nv12", rgb_frame_dtype="uint8"),
                                    dict(rgb_frame_format="nv12", rgb_frame_dtype="uint8", rgb_frame_layout="strided"),
                                    dict(rgb_frame_format="nv12", hw=(63, 96)), dict(rgb_frame_format="nv12", hw=(64, 97))])
def test_pipeline_refuses_bad_rgb_frame_format_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("mode", "rgb")
    hw = kwargs.pop("hw", (64, 96))
    with pytest.raises(ValueError, match="rgb_frame_format"):
        LineEndPipeline(hw, batch=1, **kwargs)


@pytest.mark.parametrize("kwargs,text", [(dict(nv12_matrix="bt2020"), "nv12_matrix must be"), (dict(nv12_range="video"), "nv12_range must be"),
                                         (dict(nv12_order="gbr"), "nv12_order must be"), (dict(nv12_matrix=[[1, 0], [0, 1]]), "3 x 3"),
                                         (dict(nv12_matrix=np.full((3, 3), np.nan)), "finite")])
def test_pipeline_refuses_bad_nv12_coefficients_before_any_gpu_work(kwargs, text):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match=text):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_format="nv12", **kwargs)


def test_check_rgb_frame_format():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_format
    assert chk("interleaved") == "interleaved" and chk("nv12") == "nv12" and chk("nv12", "rgb", hw=(24, 34)) == "nv12"
    # the default changes nothing, whatever the others say (they keep their own checks)
    for mode in ("gray", "rgb"):
        for rd in ("float32", "uint8"):
            for rl in ("packed", "strided"):
                for fd in ("float32", "uint8", "uint16"):
                    assert chk("interleaved", mode, rd, rl, fd, 3, "strided", (3, 5)) == "interleaved"
    for args, text in ((("nv12", "gray"), "is for mode 'rgb'"),
                       (("nv12", "rgb", "uint8"), "does not combine with rgb_frame_dtype='uint8'"),
                       (("nv12", "rgb", "float32", "strided"), "does not combine with rgb_frame_layout='strided'"),
                       (("nv12", "rgb", "float32", "packed", "uint8"), "does not combine with frame_dtype='uint8'"),
                       (("nv12", "rgb", "float32", "packed", "float32", 3), "does not combine with frame_channels=3"),
                       (("nv12", "rgb", "float32", "packed", "float32", 1, "strided"), "does not combine with frame_layout='strided'"),
                       (("nv12", "rgb", "float32", "packed", "float32", 1, "packed", (25, 34)), "needs even H and W"),
                       (("nv12", "rgb", "float32", "packed", "float32", 1, "packed", (24, 33)), "needs even H and W")):
        with pytest.raises(ValueError, match="rgb_frame_format='nv12' " + text):
            chk(*args)
    # the order: name, mode, combinations, extents
    for bad in ("yuv", None, 3, "Nv12"):
        with pytest.raises(ValueError, match="must be 'interleaved' or 'nv12'"):
            chk(bad, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))
    with pytest.raises(ValueError, match="is for mode 'rgb'"):
        chk("nv12", "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))
    with pytest.raises(ValueError, match="rgb_frame_dtype='uint8'"):
        chk("nv12", "rgb", "uint8", "strided", "uint8", 3, "strided", (3, 5))


def test_the_older_keywords_keep_their_refusals():
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match="rgb_frame_layout='strided' needs rgb_frame_dtype='uint8'"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_layout="strided", rgb_frame_format="nv12")
    with pytest.raises(ValueError, match="rgb_frame_dtype='uint8' is for mode 'rgb'"):
        LineEndPipeline((64, 96), batch=1, mode="gray", rgb_frame_dtype="uint8", rgb_frame_format="nv12")


def test_the_new_keywords_are_the_last_of_the_signature():
    import inspect
    from pysilent_amd.pipeline import LineEndPipeline
    names = list(inspect.signature(LineEndPipeline.__init__).parameters)
    assert names[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"] and names[-5] == "rgb_frame_layout"
    p = inspect.signature(LineEndPipeline.__init__).parameters
    assert [p[k].default for k in names[-4:]] == ["interleaved", "bt709", "limited", "bgr"]


def test_nv12_frames_of_and_nv12_planes():
    """The planes pass as they are: shapes, dtype, adjacency and overlap are checked, nothing is converted; nv12_planes cuts the pair out
    of surfaces [n, rows, pitch]."""
    from pysilent_amd._runtime import nv12_frames_of
    from pysilent_amd.util.zoom import nv12_planes
    n, H, W = 2, 24, 34
    y, uv = nf.batch(n, H, W)
    m, oy = nf.coefficients("bt709", "limited", "bgr")
    for fill in nf.FILLS:
        py, pu = nf.place(y, uv, fill)
        vy, vu = nf.views(py, pu, n, H, W)
        assert np.array_equal(vy, y) and np.array_equal(vu, uv)
        yr, yf, ur, uf, yo, uo, _, _ = nf.layout(n, H, W)
        args, got_n, dev = nv12_frames_of((vy, vu), (H, W), m, oy)
        assert args[:6] == (py.ctypes.data + yo, pu.ctypes.data + uo, yr, yf, ur, uf) and got_n == n and not dev
        assert np.array_equal(np.array(args[6], np.float32), m.reshape(9)) and args[7] == 16.0
    for bad, text in (((vy, vu[:, :, :, ::-1]), "adjacent"), ((vy[:, :, ::-1], vu), "adjacent"), ((vy.astype(np.float32), vu), "uint8"),
                      ((vy, vu[:1]), "chroma plane"), ((vy[:, :23], vu), "luma plane"), ((vy[:, ::-1], vu), "overlap"),
                      ((np.broadcast_to(vy[:1], vy.shape), vu), "overlap"), ((vy, vu, vu), "pair"), (vy, "pair")):
        with pytest.raises(ValueError, match=text):
            nv12_frames_of(bad, (H, W), m, oy)
    surf = np.random.default_rng(5).integers(0, 256, (3, 40, 64)).astype(np.uint8)
    sy, su = nv12_planes(surf, H, W)
    assert np.array_equal(sy, surf[:, :H, :W]) and su.shape == (3, H // 2, W // 2, 2)
    assert np.array_equal(su.reshape(3, H // 2, W), surf[:, H:H + H // 2, :W]) and np.shares_memory(su, surf) and np.shares_memory(sy, surf)
    args, _, _ = nv12_frames_of((sy, su), (H, W), m, oy)
    assert args[:6] == (surf.ctypes.data, surf.ctypes.data + H * 64, 64, 40 * 64, 64, 40 * 64)
    lower = nv12_planes(surf, H, W, chroma_row=28)[1]
    assert np.array_equal(lower.reshape(3, H // 2, W), surf[:, 28:40, :W])
    for bad in (dict(H=23), dict(W=33), dict(chroma_row=29), dict(chroma_row=20)):
        with pytest.raises(ValueError, match="nv12_planes"):
            nv12_planes(surf, **dict(dict(H=H, W=W), **bad))


# ----------------------------------------------------------------------------- the ABI

def test_nv12_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert "const silent_nv12_frames* frames" in " ".join(src[src.index("int " + name + "("):].split(";")[0].split()), name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["silent_pyramid_nv12"] == [vp, vp, _lib._np, i, vp]
    assert _lib._SIGNATURES["silent_pyramid_nv12_dev"] == _lib._SIGNATURES["silent_pyramid_nv12"] + [vp]
    assert _lib._SIGNATURES["silent_nv12_to_rgb"] == [vp, _lib._np, i, i, i, vp]
    assert _lib._SIGNATURES["silent_nv12_to_rgb_dev"] == _lib._SIGNATURES["silent_nv12_to_rgb"] + [vp]
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src


def test_the_ctypes_struct_matches_the_header():
    """Field names, order and types of silent_nv12_frames as the header declares them; offsets and size as the C compiler lays out two
    pointers, four int64, nine floats and one float."""
    from pysilent_amd import _lib
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    body = src[src.index("typedef struct silent_nv12_frames {") + len("typedef struct silent_nv12_frames {"):src.index("} silent_nv12_frames;")]
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.rsplit(" ", decl.count(",") + 1)[0], decl.split(" ", decl.count(" ") - decl.count(","))[-1]
        for name in names.split(","):
            fields.append((name.strip(), ctype))
    assert fields == [("y", "const uint8_t*"), ("uv", "const uint8_t*"), ("y_row_stride", "int64_t"), ("y_frame_stride", "int64_t"),
                      ("uv_row_stride", "int64_t"), ("uv_frame_stride", "int64_t"), ("m[9]", "float"), ("oy", "float")]
    S = _lib.Nv12Frames
    assert [f[0] for f in S._fields_] == [n.split("[")[0] for n, _ in fields]
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 84] and ctypes.sizeof(S) == 88
    p = _lib.nv12_ptr((1, 2, 3, 4, 5, 6, list(range(9)), 16.0)).contents
    assert (p.y, p.uv, p.y_row_stride, p.y_frame_stride, p.uv_row_stride, p.uv_frame_stride, list(p.m), p.oy) == (1, 2, 3, 4, 5, 6, list(range(9)), 16.0)
    assert _lib.nv12_ptr(None) is None


def test_library_exports_the_nv12_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


def test_launch_summary_and_byte_accounting_of_an_nv12_pipeline():
    """The summary says "NV12 read in place"; the frame counts 1.5 bytes per pixel; everything else is the float32 RGB pipeline's."""
    from test_rgb_uint8_host import _accounting_pipeline
    h, w = 1080, 1920
    f32, nv = _accounting_pipeline((h, w), "float32", 6), _accounting_pipeline((h, w), "float32", 6)
    nv.rgb_frame_format = "nv12"
    assert "NV12 read in place" in nv.launch_summary() and "NV12" not in f32.launch_summary()
    assert nv.launch_summary().startswith(f32.launch_summary())
    assert nv._frame_bytes * 3 == 1.5 and f32._frame_bytes == 4
    assert nv.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 12 * h * w + h * w * 3 // 2
    assert nv.pyramid_bytes_per_frame() == f32.pyramid_bytes_per_frame() - 12 * h * w + h * w * 3 // 2
    assert nv.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    assert isinstance(nv.algorithmic_bytes_per_frame(), int) and isinstance(nv.pyramid_bytes_per_frame(), int)
    assert nv.dominant_kernel_name() == f32.dominant_kernel_name()


# ----------------------------------------------------------------------------- the conversion

@pytest.mark.parametrize("matrix,rng,order", nf.VARIANTS, ids=["-".join(v) for v in nf.VARIANTS])
def test_the_named_matrices_equal_their_closed_forms(matrix, rng, order):
    from pysilent_amd._runtime import nv12_coefficients
    m, oy = nv12_coefficients(matrix, rng, order)
    want, want_oy = nf.coefficients(matrix, rng, order)
    assert m.dtype == np.float32 and m.shape == (3, 3) and np.array_equal(m, want) and oy == want_oy and type(oy) is np.float32
    # the closed forms once more, written out: R, G, B rows over (Y', U', V')
    kr, kb = {"bt601": (.299, .114), "bt709": (.2126, .0722)}[matrix]
    ys, cs = (255 / 219, 255 / 224) if rng == "limited" else (1.0, 1.0)
    rgb = m if order == "rgb" else m[::-1]
    f = np.float32
    assert np.array_equal(rgb[:, 0], [f(ys)] * 3)
    assert rgb[0, 1] == 0 and rgb[0, 2] == f(2 * (1 - kr) * cs) and rgb[2, 1] == f(2 * (1 - kb) * cs) and rgb[2, 2] == 0
    assert rgb[1, 1] == f(-2 * kb * (1 - kb) / (1 - kr - kb) * cs) and rgb[1, 2] == f(-2 * kr * (1 - kr) / (1 - kr - kb) * cs)
    assert oy == (16 if rng == "limited" else 0)
    # white, black and the primaries' luma land where the standard puts them (to float32 rounding of three products and two sums)
    lo, hi = (16, 235) if rng == "limited" else (0, 255)
    grey = nf.convert_yuv(np.array([lo, hi], np.uint8), np.array([128, 128], np.uint8), np.array([128, 128], np.uint8), m, oy)
    assert np.array_equal(grey[0], [0, 0, 0]) and np.allclose(grey[1], 255, atol=1e-4)


def test_a_matrix_given_as_an_array_is_taken_as_it_is():
    from pysilent_amd._runtime import nv12_coefficients
    a = np.arange(9, dtype=np.float64).reshape(3, 3) / 7
    m, oy = nv12_coefficients(a, "full", "rgb")
    assert np.array_equal(m, a.astype(np.float32)) and oy == 0
    assert nv12_coefficients(a.tolist(), "limited")[1] == 16


def test_the_restatement_is_pinned_on_the_recorded_case():
    """All 256 Y values with a 16 x 16 grid of (U, V) (nf.combinations, one 256 x 256 frame): the SHA-256 of the restatement's float32
    output for each matrix / range / order, and the output itself for the first four rows under bt709 / limited / bgr."""
    y, uv = nf.combinations()
    assert sorted(set(y.ravel().tolist())) == list(range(256)) and len({tuple(p) for p in uv.reshape(-1, 2).tolist()}) == 256
    seen = {(int(a), int(u), int(v)) for a, (u, v) in zip(y[0].ravel(), np.repeat(np.repeat(uv[0], 2, 0), 2, 1).reshape(-1, 2))}
    assert len(seen) == 256 * 256
    recorded = dict(l.rsplit(" ", 1) for l in open(os.path.join(GOLDEN, "nv12_convert_sha256.txt")).read().strip().split("\n"))
    assert len(recorded) == 8
    for v in nf.VARIANTS:
        m, oy = nf.coefficients(*v)
        out = nf.convert(y, uv, m, oy)
        assert out.dtype == np.float32 and out.min() >= 0 and out.max() <= 255
        assert nf.digest(out) == recorded[" ".join(v)], v
    rows = np.load(os.path.join(GOLDEN, "nv12_convert_bt709_limited_bgr_rows0_3.npy"))
    m, oy = nf.coefficients("bt709", "limited", "bgr")
    assert np.array_equal(nf.convert(y, uv, m, oy)[0, :4].view(np.uint32), rows.view(np.uint32))
    # not rounded to integers, and the clamp acts
    assert np.any(rows != np.round(rows)) and np.any(rows == 0) and np.any(nf.convert(y, uv, m, oy) == 255)


def test_separate_roundings_differ_from_a_fused_multiply_add():
    """What the restatement pins is the order and the separate roundings: summing in float64 and rounding once (what an FMA chain
    approaches) gives other bits on the recorded case."""
    y, uv = nf.combinations()
    m, oy = nf.coefficients("bt709", "limited", "bgr")
    Y, U, V = (a.astype(np.float64) for a in (y, np.repeat(np.repeat(uv[..., 0], 2, 1), 2, 2), np.repeat(np.repeat(uv[..., 1], 2, 1), 2, 2)))
    once = np.stack([np.clip((Y - 16) * float(m[k, 0]) + (U - 128) * float(m[k, 1]) + (V - 128) * float(m[k, 2]), 0, 255) for k in range(3)], -1)
    got = nf.convert(y, uv, m, oy)
    assert np.max(np.abs(got - once)) < 1e-3 and np.count_nonzero(got != once.astype(np.float32)) > 1000


# ----------------------------------------------------------------------------- what the frames can see

N, H, W = 2, 24, 34


@pytest.fixture(scope="module")
def correct_pyramid():
    y, uv = nf.batch(N, H, W)
    m, oy = nf.coefficients("bt709", "limited", "bgr")
    frames = nf.convert(y, uv, m, oy)
    return (y, uv, m, oy), frames, [so.classic_pyramid(f, 2.0, 2) for f in frames]


def _beyond_assert_close(got, want, what):
    """True when conftest.assert_close, with the rounding bound of the zoom, refuses ``got`` for ``want`` on some level."""
    for l, (g, w) in enumerate(zip(got, want)):
        try:
            assert_close(g.astype(np.float32), w, 1e-5, scale=255.0, what="%s level %d" % (what, l), bound=eb.zoom(w))
        except AssertionError:
            return True
    return False


def test_the_surfaces_carry_the_batch_under_both_fills(correct_pyramid):
    (y, uv, m, oy), frames, want = correct_pyramid
    yr, yf, ur, uf = nf.layout(N, H, W)[:4]
    assert yr != ur and yf != H * yr and uf != (H // 2) * ur
    for fill in nf.FILLS:
        py, pu = nf.place(y, uv, fill)
        seen = nf.truth(py, pu, N, H, W, m, oy)
        assert np.array_equal(seen.view(np.uint32), frames.view(np.uint32))
        my, mu = nf.pixel_mask(N, H, W)
        assert np.all(py[~my] == fill) and np.all(pu[~mu] == fill) and my.sum() == N * H * W and mu.sum() == N * H * W // 2
        assert not _beyond_assert_close(so.classic_pyramid(seen[1], 2.0, 2), want[1], "truth")


@pytest.mark.parametrize("name", sorted(nf.MISTAKES))
def test_the_surfaces_separate_each_mistake_from_the_truth(correct_pyramid, name):
    """The oracle's pyramid of what a mistaken loader would see differs from the true one by more than assert_close allows, under at
    least one of the two fills, on every frame where the mistake acts (frame 1 for the frame stride)."""
    (y, uv, m, oy), frames, want = correct_pyramid
    shown = False
    for fill in nf.FILLS:
        py, pu = nf.place(y, uv, fill)
        seen = nf.MISTAKES[name](py, pu, N, H, W, m, oy)
        assert seen.shape == frames.shape and seen.dtype == np.float32
        shown = shown or all(_beyond_assert_close(so.classic_pyramid(seen[f], 2.0, 2), want[f], name) for f in nf.FRAMES_HIT.get(name, (0, 1)))
    assert shown, "%s is invisible on these frames" % name


# ----------------------------------------------------------------------------- the host side under the sanitizers

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@needs_hipcc
def test_nv12_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Both forms of both entry points on 40 x 58 surfaces whose planes are heap blocks of exactly their spans, for a classic and a crop
    plan; the staged bytes are the two spans and the poisoned arena behind them is untouched; the status codes and the order of the
    checks.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb nv12 host main ok" in run_driver("rgb_nv12")


@needs_hipcc
def test_every_single_fault_of_the_nv12_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb_nv12", "--refusals").strip().split("\n")
    want = open(os.path.join(GOLDEN, "nv12_refusals.txt")).read().strip().split("\n")
    assert len(want) == 2 * 18 + 2 * 15 and {l.split(" | ")[0] for l in want} == set(NAMES)
    assert got == want
    for l in want:
        name, case, status, text = l.split(" | ")
        assert text.startswith(name.replace("_dev", "") + ": "), l
        assert status == ("-4" if case == "single-channel plan" else "-1"), l
    single = [l for l in want if "single-channel plan" in l]
    assert len(single) == 2 and all("silent_pyramid_view)" in l for l in single)
    assert sum("even H and W" in l for l in want) == 8 and sum("must be finite" in l for l in want) == 8


E5 = math.e ** .5


def odd_origin_crops(hw=(270, 482)):
    """A crop layout whose innermost crop starts at an odd row AND an odd column of the frame, the centre size chosen here: only such a
    plan separates the chroma sample (x0 + x) >> 1 from x0 / 2 + x / 2 (and the same for rows)."""
    from pysilent_amd.util.zoom.from_image import reference_levels
    for cw in range(44, 64):
        for ch in range(60, 80):
            levels = reference_levels(hw, (cw, ch), 2.0)
            if len(levels) >= 3 and levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1:
                return hw, (cw, ch), levels
    raise AssertionError("no centre size gives an odd origin")


def _address_plans():
    from pysilent_amd.util.zoom.from_image import classic_levels
    return [((40, 8), classic_levels((40, 8), 2.0, 2)), ((64, 66), classic_levels((64, 66), 2.0, 3)),
            ((134, 242), classic_levels((134, 242), 2.0, 4)), odd_origin_crops()[::2]]


@needs_hipcc
@pytest.mark.parametrize("which", range(4), ids=["classic-40x8", "classic-64x66", "classic-134x242", "crops-270x482"])
def test_every_address_of_the_walk_loader_lies_inside_its_span_and_covers_the_crops(which):
    """--addresses: w3_nv12_load -- the function pyramid_walk3_kernel forms its NV12 loads with -- for every block, chunk, row, lane and
    load slot of the plan's launch on two frames: no access outside the luma span or the chroma span, every Y byte of every crop pixel
    and both bytes of the pair under it among the bytes touched, no byte touched that is not a pixel's."""
    from test_gray_uint8_host import run_driver
    hw, levels = _address_plans()[which]
    out = run_driver("rgb_nv12", "--addresses", str(hw[0]), str(hw[1]), str(len(levels)), *[str(int(v)) for l in levels for v in l])
    lines = [l for l in out.strip().split("\n") if l]
    assert len(lines) == 1, out
    f = lines[0].split(" | ")
    assert f[0] == "%d x %d" % hw and f[3] == "outside 0" and f[4].endswith("missing y 0 uv 0") and f[5] == "not a pixel byte 0", lines[0]
    assert int(f[4].split()[1]) > 0 and int(f[2].split()[1]) > 0, lines[0]
    if which == 3:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
        assert "plans 2 " in f[1] and int(f[6].split()[2]) >= 1, lines[0]
