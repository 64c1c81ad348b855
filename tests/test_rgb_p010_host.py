"""P010 / P012 / P016 decoder surfaces for 3-channel plans (rgb_frame_format="p010" / "p012" / "p016", silent_pyramid_p010[_dev],
silent_p010_to_rgb[_dev]) without a GPU: the keyword's refusals (before any torch or GPU work), the symbols and the struct, the
coefficients against their closed forms, the NumPy restatement of the conversion -- its identity with the NV12 restatement on
(byte << 8) | junk, the low bits, the fused form, the extremes, a recorded case -- what the test frames can see (each mistake a P010
loader can make moves the oracle's pyramid beyond conftest.assert_close), the byte accounting, and the host side of the entry points --
argument validation, the refusal table, the host forms' staging of exactly the two spans, and the walk loader's address function
enumerated over whole launches -- as a stand-alone program (tests/rgb_p010_host_main.cpp) built with the library's host side under
ASan + UBSan and run as a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
import rgb_p010_frames as pf
import silent_oracle as so
from conftest import ROOT, assert_close

NAMES = ("silent_pyramid_p010", "silent_pyramid_p010_dev", "silent_p010_to_rgb", "silent_p010_to_rgb_dev")
FORMATS = {"p010": 10, "p012": 12, "p016": 16}
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ----------------------------------------------------------------------------- the keyword

UNKNOWN = "rgb_frame_format must be 'interleaved' or 'nv12', or 'p010' / 'p012' / 'p016'"


@pytest.mark.parametrize("kwargs,text", [(dict(rgb_frame_format="P010"), UNKNOWN), (dict(rgb_frame_format="p014"), UNKNOWN), (dict(rgb_frame_format=10), UNKNOWN),
                                         (dict(rgb_frame_format="p010", mode="gray"), "^rgb_frame_format='p010' is for mode 'rgb'"),
                                         (dict(rgb_frame_format="p012", rgb_frame_dtype="uint8"), "^rgb_frame_format='p012' does not combine with rgb_frame_dtype"),
                                         (dict(rgb_frame_format="p016", rgb_frame_dtype="uint8", rgb_frame_layout="strided"), "^rgb_frame_format='p016' does not combine with rgb_frame_dtype"),
                                         (dict(rgb_frame_format="p010", hw=(63, 96)), "^rgb_frame_format='p010' needs even H and W"),
                                         (dict(rgb_frame_format="p016", hw=(64, 97)), "^rgb_frame_format='p016' needs even H and W")])
def test_pipeline_refuses_bad_p010_formats_before_any_gpu_work(kwargs, text):
    from pysilent_amd.pipeline import LineEndPipeline
    kwargs.setdefault("mode", "rgb")
    hw = kwargs.pop("hw", (64, 96))
    with pytest.raises(ValueError, match=text):
        LineEndPipeline(hw, batch=1, **kwargs)


@pytest.mark.parametrize("kwargs,text", [(dict(nv12_matrix="bt2100"), "nv12_matrix must be 'bt601', 'bt709', 'bt2020'"), (dict(nv12_range="video"), "nv12_range must be"),
                                         (dict(nv12_order="gbr"), "nv12_order must be"), (dict(nv12_matrix=[[1, 0], [0, 1]]), "3 x 3"),
                                         (dict(nv12_matrix=np.full((3, 3), np.nan)), "finite")])
def test_pipeline_refuses_bad_p010_coefficients_before_any_gpu_work(kwargs, text):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match=text):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_format="p010", **kwargs)


def test_bt2020_is_for_the_wide_formats_only():
    """"bt2020" passes the coefficient check of every P010 format and is still refused with "nv12", with the text NV12 has."""
    from pysilent_amd import _runtime
    from pysilent_amd.pipeline import LineEndPipeline
    for fmt, depth in FORMATS.items():
        m, oy, oc = _runtime.p010_coefficients("bt2020", "limited", "bgr", depth)
        assert np.array_equal(m, pf.coefficients("bt2020", "limited", "bgr", depth)[0])
    with pytest.raises(ValueError, match="nv12_matrix must be 'bt601', 'bt709' or a 3 x 3 array, got 'bt2020'"):
        _runtime.nv12_coefficients("bt2020")
    with pytest.raises(ValueError, match="nv12_matrix must be 'bt601', 'bt709' or a 3 x 3 array, got 'bt2020'"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", rgb_frame_format="nv12", nv12_matrix="bt2020")
    with pytest.raises(ValueError, match="nv12_matrix must be 'bt601', 'bt709' or a 3 x 3 array, got 'bt2020'"):
        LineEndPipeline((64, 96), batch=1, mode="rgb", nv12_matrix="bt2020")
    assert "bt2020" not in _runtime.NV12_MATRICES and "bt2020" in _runtime.P010_MATRICES


def test_check_rgb_frame_format_for_the_new_names():
    from pysilent_amd import _runtime
    chk = _runtime.check_rgb_frame_format
    assert _runtime.RGB_FRAME_FORMATS == ("interleaved", "nv12", "p010", "p012", "p016")
    assert _runtime.P010_DEPTHS == FORMATS
    for fmt in FORMATS:
        assert chk(fmt) == fmt and chk(fmt, "rgb", hw=(24, 34)) == fmt
        for args, text in (((fmt, "gray"), "is for mode 'rgb'"),
                           ((fmt, "rgb", "uint8"), "does not combine with rgb_frame_dtype='uint8'"),
                           ((fmt, "rgb", "float32", "strided"), "does not combine with rgb_frame_layout='strided'"),
                           ((fmt, "rgb", "float32", "packed", "uint16"), "does not combine with frame_dtype='uint16'"),
                           ((fmt, "rgb", "float32", "packed", "float32", 3), "does not combine with frame_channels=3"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "strided"), "does not combine with frame_layout='strided'"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "packed", (25, 34)), "needs even H and W"),
                           ((fmt, "rgb", "float32", "packed", "float32", 1, "packed", (24, 33)), "needs even H and W")):
            with pytest.raises(ValueError, match="^rgb_frame_format='%s' %s" % (fmt, text)):
                chk(*args)
        # the order: name, mode, combinations, extents
        with pytest.raises(ValueError, match="is for mode 'rgb'"):
            chk(fmt, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))
        with pytest.raises(ValueError, match="rgb_frame_dtype='uint8'"):
            chk(fmt, "rgb", "uint8", "strided", "uint8", 3, "strided", (3, 5))
        with pytest.raises(ValueError, match="rgb_frame_layout='strided'"):
            chk(fmt, "rgb", "float32", "strided", "uint8", 3, "strided", (3, 5))
        with pytest.raises(ValueError, match="even H and W"):
            chk(fmt, "rgb", "float32", "packed", "float32", 1, "packed", (3, 5))
    # an unknown name: the text the NV12 tests match, with the new names behind it
    for bad in ("yuv", None, 3, "P010", "p014"):
        with pytest.raises(ValueError, match="must be 'interleaved' or 'nv12'.*'p010' / 'p012' / 'p016'"):
            chk(bad, "gray", "uint8", "strided", "uint8", 3, "strided", (3, 5))


def test_the_formats_are_values_of_the_keyword_and_the_signature_is_unchanged():
    """No new keyword: the depth is in the format's name."""
    import inspect
    from pysilent_amd import _runtime
    assert _runtime.RGB_FRAME_FORMATS[-3:] == ("p010", "p012", "p016")
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd._runtime import PyramidPlan
    names = list(inspect.signature(LineEndPipeline.__init__).parameters)
    assert names[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"] and names[-5] == "rgb_frame_layout"
    assert not any("p010" in k or "depth" in k for k in names)
    assert list(inspect.signature(PyramidPlan.run).parameters)[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"]


def test_p010_frames_of_and_p010_planes():
    """The planes pass as they are: shapes, dtype, adjacency and overlap are checked, strides are BYTES, nothing is converted;
    p010_planes cuts the pair out of uint16 surfaces [n, rows, pitch_elements]."""
    from pysilent_amd._runtime import p010_frames_of
    from pysilent_amd.util.zoom import p010_planes
    n, H, W = 2, 24, 34
    y, uv = pf.batch(n, H, W)
    m, oy, oc = pf.coefficients("bt709", "limited", "bgr", 10)
    for fill in pf.FILLS:
        py, pu = pf.place(y, uv, fill)
        vy, vu = pf.views(py, pu, n, H, W)
        assert np.array_equal(vy, y) and np.array_equal(vu, uv)
        yr, yf, ur, uf, yo, uo, _, _ = pf.layout(n, H, W)
        args, got_n, dev = p010_frames_of((vy, vu), (H, W), m, oy, oc, 10)
        assert args[:6] == (py.ctypes.data + 2 * yo, pu.ctypes.data + 2 * uo, 2 * yr, 2 * yf, 2 * ur, 2 * uf) and got_n == n and not dev
        assert np.array_equal(np.array(args[6], np.float32), m.reshape(9)) and args[7:] == (64.0, 512.0, 6)
        assert pu.ctypes.data % 4 == 0 and args[1] % 4 == 2          # the chroma plane starts at an address that is 2 (mod 4)
    assert p010_frames_of((vy, vu), (H, W), m, oy, oc, 12)[0][9] == 4 and p010_frames_of((vy, vu), (H, W), m, oy, oc, 16)[0][9] == 0
    for bad, text in (((vy, vu[:, :, :, ::-1]), "adjacent"), ((vy[:, :, ::-1], vu), "adjacent"), ((vy.astype(np.float32), vu), "uint16"),
                      ((vy.astype(np.uint8), vu), "uint16"), ((vy, vu.astype(np.int16)), "uint16"),
                      ((vy, vu[:1]), "chroma plane"), ((vy[:, :23], vu), "luma plane"), ((vy[:, ::-1], vu), "overlap"),
                      ((np.broadcast_to(vy[:1], vy.shape), vu), "overlap"), ((vy, vu, vu), "pair"), (vy, "pair")):
        with pytest.raises(ValueError, match=text):
            p010_frames_of(bad, (H, W), m, oy, oc, 10)
    with pytest.raises(ValueError, match="depth must be"):
        p010_frames_of((vy, vu), (H, W), m, oy, oc, 8)
    surf = np.random.default_rng(5).integers(0, 65536, (3, 40, 64)).astype(np.uint16)
    sy, su = p010_planes(surf, H, W)
    assert np.array_equal(sy, surf[:, :H, :W]) and su.shape == (3, H // 2, W // 2, 2)
    assert np.array_equal(su.reshape(3, H // 2, W), surf[:, H:H + H // 2, :W]) and np.shares_memory(su, surf) and np.shares_memory(sy, surf)
    args, _, _ = p010_frames_of((sy, su), (H, W), m, oy, oc, 10)
    assert args[:6] == (surf.ctypes.data, surf.ctypes.data + H * 128, 128, 40 * 128, 128, 40 * 128)
    lower = p010_planes(surf, H, W, chroma_row=28)[1]
    assert np.array_equal(lower.reshape(3, H // 2, W), surf[:, 28:40, :W])
    for bad in (dict(H=23), dict(W=33), dict(chroma_row=29), dict(chroma_row=20), dict(surfaces=surf.astype(np.uint8))):
        with pytest.raises(ValueError, match="p010_planes"):
            p010_planes(**dict(dict(surfaces=surf, H=H, W=W), **bad))


# ----------------------------------------------------------------------------- the ABI

def test_p010_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
        assert "const silent_p010_frames* frames" in " ".join(src[src.index("int " + name + "("):].split(";")[0].split()), name
        # the argument list of the NV12 twin
        twin = name.replace("p010", "nv12")
        own, other = (" ".join(src[src.index("int " + k + "("):].split(";")[0].split()) for k in (name, twin))
        assert own.replace("p010", "nv12") == other, name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["silent_pyramid_p010"] == [vp, vp, _lib._pp, i, vp]
    assert _lib._SIGNATURES["silent_pyramid_p010_dev"] == _lib._SIGNATURES["silent_pyramid_p010"] + [vp]
    assert _lib._SIGNATURES["silent_p010_to_rgb"] == [vp, _lib._pp, i, i, i, vp]
    assert _lib._SIGNATURES["silent_p010_to_rgb_dev"] == _lib._SIGNATURES["silent_p010_to_rgb"] + [vp]
    assert _lib.ABI_VERSION == 5 and "#define SILENT_ABI_VERSION 5" in src


def test_the_ctypes_struct_matches_the_header():
    """Field names, order and types of silent_p010_frames as the header declares them; offsets and size as the C compiler lays out two
    pointers, four int64, nine floats, two floats and an int."""
    from pysilent_amd import _lib
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    body = src[src.index("typedef struct silent_p010_frames {") + len("typedef struct silent_p010_frames {"):src.index("} silent_p010_frames;")]
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.rsplit(" ", decl.count(",") + 1)[0], decl.split(" ", decl.count(" ") - decl.count(","))[-1]
        for name in names.split(","):
            fields.append((name.strip(), ctype))
    assert fields == [("y", "const uint16_t*"), ("uv", "const uint16_t*"), ("y_row_stride", "int64_t"), ("y_frame_stride", "int64_t"),
                      ("uv_row_stride", "int64_t"), ("uv_frame_stride", "int64_t"), ("m[9]", "float"), ("oy", "float"), ("oc", "float"),
                      ("shift", "int")]
    S = _lib.P010Frames
    assert [f[0] for f in S._fields_] == [n.split("[")[0] for n, _ in fields]
    ctypes_of = {"const uint16_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
    for (name, ctype), (_, got) in zip(fields, S._fields_):
        assert got == (ctypes.c_float * 9 if name == "m[9]" else ctypes_of[ctype]), name
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 84, 88, 92] and ctypes.sizeof(S) == 96
    p = _lib.p010_ptr((2, 4, 6, 8, 10, 12, list(range(9)), 64.0, 512.0, 6)).contents
    assert (p.y, p.uv, p.y_row_stride, p.y_frame_stride, p.uv_row_stride, p.uv_frame_stride, list(p.m), p.oy, p.oc, p.shift) == \
        (2, 4, 6, 8, 10, 12, list(range(9)), 64.0, 512.0, 6)
    assert _lib.p010_ptr(None) is None


def test_library_exports_the_p010_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.silent_abi_version() == 5


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_launch_summary_and_byte_accounting_of_a_p010_pipeline(fmt):
    """The summary says "P010 read in place" with the format's name; the frame counts 3 bytes per pixel (NV12 keeps 1.5); everything
    else is the float32 RGB pipeline's."""
    from test_rgb_uint8_host import _accounting_pipeline
    h, w = 1080, 1920
    f32, pp, nv = (_accounting_pipeline((h, w), "float32", 6) for _ in range(3))
    pp.rgb_frame_format, nv.rgb_frame_format = fmt, "nv12"
    assert "%s read in place" % fmt.upper() in pp.launch_summary() and "read in place" not in f32.launch_summary()
    assert "NV12" not in pp.launch_summary() and pp.launch_summary().startswith(f32.launch_summary())
    assert pp._frame_bytes == 1.0 and pp._frame_bytes * 3 == 3 and nv._frame_bytes == 0.5 and f32._frame_bytes == 4
    assert pp._p010 == FORMATS[fmt] and not pp._nv12 and nv._p010 is None and f32._p010 is None
    assert pp.algorithmic_bytes_per_frame() == f32.algorithmic_bytes_per_frame() - 12 * h * w + 3 * h * w
    assert pp.pyramid_bytes_per_frame() == f32.pyramid_bytes_per_frame() - 12 * h * w + 3 * h * w
    assert pp.filter_bytes_per_frame() == f32.filter_bytes_per_frame()
    assert isinstance(pp.algorithmic_bytes_per_frame(), int) and isinstance(pp.pyramid_bytes_per_frame(), int)
    assert pp.dominant_kernel_name() == f32.dominant_kernel_name()


# ----------------------------------------------------------------------------- the conversion

def _coefficients(matrix, rng, order, depth):
    """(m, oy, oc) of the LIBRARY (_runtime.p010_coefficients), which are those of the closed forms: the restatement below is run
    with the numbers the kernels get."""
    from pysilent_amd._runtime import p010_coefficients
    got, want = p010_coefficients(matrix, rng, order, depth), pf.coefficients(matrix, rng, order, depth)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    return got


@pytest.mark.parametrize("depth", pf.DEPTHS)
@pytest.mark.parametrize("matrix,rng,order", pf.VARIANTS, ids=["-".join(v) for v in pf.VARIANTS])
def test_the_named_matrices_equal_their_closed_forms(matrix, rng, order, depth):
    from pysilent_amd._runtime import p010_coefficients
    m, oy, oc = p010_coefficients(matrix, rng, order, depth)
    want, want_oy, want_oc = pf.coefficients(matrix, rng, order, depth)
    assert m.dtype == np.float32 and m.shape == (3, 3) and np.array_equal(m, want)
    assert oy == want_oy and oc == want_oc and type(oy) is np.float32 and type(oc) is np.float32
    # the closed forms once more, written out: R, G, B rows over (Y', U', V')
    kr, kb = {"bt601": (.299, .114), "bt709": (.2126, .0722), "bt2020": (.2627, .0593)}[matrix]
    s = 2 ** (depth - 8)
    ys, cs = (255 / (219 * s), 255 / (224 * s)) if rng == "limited" else (255 / (2 ** depth - 1),) * 2
    rgb = m if order == "rgb" else m[::-1]
    f = np.float32
    assert np.array_equal(rgb[:, 0], [f(ys)] * 3)
    assert rgb[0, 1] == 0 and rgb[0, 2] == f(2 * (1 - kr) * cs) and rgb[2, 1] == f(2 * (1 - kb) * cs) and rgb[2, 2] == 0
    assert rgb[1, 1] == f(-2 * kb * (1 - kb) / (1 - kr - kb) * cs) and rgb[1, 2] == f(-2 * kr * (1 - kr) / (1 - kr - kb) * cs)
    assert oy == (16 * s if rng == "limited" else 0) and oc == 128 * s
    if rng == "limited" and matrix != "bt2020":
        # m s is the NV12 matrix exactly (a power of two)
        assert np.array_equal(m * f(s), nf.coefficients(matrix, rng, order)[0])


@pytest.mark.parametrize("depth", pf.DEPTHS)
def test_a_matrix_given_as_an_array_is_scaled_by_the_power_of_two_exactly(depth):
    from pysilent_amd._runtime import p010_coefficients
    a = np.arange(9, dtype=np.float64).reshape(3, 3) / 7
    m, oy, oc = p010_coefficients(a, "full", "rgb", depth)
    s = 2 ** (depth - 8)
    assert np.array_equal(m * np.float32(s), a.astype(np.float32)) and np.array_equal(m, (a.astype(np.float32).astype(np.float64) / s).astype(np.float32))
    assert oy == 0 and oc == 128 * s
    assert p010_coefficients(a.tolist(), "limited", depth=depth)[1] == 16 * s
    with pytest.raises(ValueError, match="depth must be"):
        p010_coefficients(a, depth=8)


@pytest.mark.parametrize("depth", pf.DEPTHS)
def test_the_conversion_of_shifted_bytes_is_the_nv12_conversion_bit_for_bit(depth):
    """Limited range, (byte << 8) | junk with junk in the low 16 - depth bits: the P010 restatement with the depth's coefficients gives
    the bits the NV12 restatement gives for the bytes -- bt601 / bt709 x bgr / rgb on 200 000 random triples."""
    rng = np.random.default_rng(77 + depth)
    shift = 16 - depth
    Y, U, V = (rng.integers(0, 256, 200000).astype(np.uint8) for _ in range(3))
    wide = [((b.astype(np.uint16) << 8) | (rng.integers(0, 1 << shift, b.shape) if shift else 0)).astype(np.uint16) for b in (Y, U, V)]
    if shift:
        assert all(np.any(w & ((1 << shift) - 1)) for w in wide)
    for matrix in ("bt601", "bt709"):
        for order in ("bgr", "rgb"):
            m8, oy8 = nf.coefficients(matrix, "limited", order)
            m, oy, oc = _coefficients(matrix, "limited", order, depth)
            got = pf.convert_yuv(wide[0], wide[1], wide[2], m, oy, oc, shift)
            assert np.array_equal(got.view(np.uint32), nf.convert_yuv(Y, U, V, m8, oy8).view(np.uint32)), (matrix, order)


@pytest.mark.parametrize("depth", (10, 12))
def test_the_low_bits_change_no_result(depth):
    shift = 16 - depth
    y, uv = pf.batch(2, 24, 34, depth)
    m, oy, oc = _coefficients("bt2020", "limited", "rgb", depth)
    want = pf.convert(y, uv, m, oy, oc, shift)
    low = np.uint16((1 << shift) - 1)
    for fy, fu in ((y ^ low, uv ^ low), (y & ~low, uv & ~low), (y | low, uv | low)):
        assert np.array_equal(pf.convert(fy, fu, m, oy, oc, shift).view(np.uint32), want.view(np.uint32))
    assert np.any(y & low) and np.any(uv & low)                    # (the test data has junk there)
    assert not np.array_equal(pf.convert(y ^ np.uint16(1 << shift), uv, m, oy, oc, shift), want)   # (the lowest bit of the code counts)


def test_separate_roundings_differ_from_a_fused_multiply_add():
    """What the restatement pins is the order and the separate roundings: a fused multiply-add chain -- each product exact, one
    rounding per accumulation step, here in float64 -- gives other bits on the test data."""
    y, uv = pf.combinations10()
    m, oy, oc = _coefficients("bt709", "limited", "bgr", 10)
    got = pf.convert(y, uv, m, oy, oc, 6)
    f = np.float32
    Yc, Uc, Vc = ((a >> 6).astype(np.float64) for a in (y, np.repeat(np.repeat(uv[..., 0], 2, 1), 2, 2), np.repeat(np.repeat(uv[..., 1], 2, 1), 2, 2)))
    fused = []
    for k in range(3):
        a = ((Yc - 64) * float(m[k, 0])).astype(f)                                       # rounded product
        a = (a.astype(np.float64) + (Uc - 512) * float(m[k, 1])).astype(f)               # fma: exact product, one rounding
        a = (a.astype(np.float64) + (Vc - 512) * float(m[k, 2])).astype(f)               # fma
        fused.append(np.clip(a, 0, 255))
    fused = np.stack(fused, -1)
    differ = np.count_nonzero(np.any(got != fused, -1)) / got[..., 0].size
    assert np.max(np.abs(got - fused)) < 1e-3 and differ > 0.05, differ


@pytest.mark.parametrize("depth", pf.DEPTHS)
def test_the_extremes_land_where_the_standards_put_them(depth):
    shift, s, top = 16 - depth, 2 ** (depth - 8), 2 ** depth - 1
    e = lambda *codes: (np.array(codes, np.int64) << shift).astype(np.uint16)
    for matrix, _, order in pf.VARIANTS[::2]:
        m, oy, oc = _coefficients(matrix, "full", order, depth)
        out = pf.convert_yuv(e(0, top), e(128 * s, 128 * s), e(128 * s, 128 * s), m, oy, oc, shift)
        assert np.array_equal(out[0], [0, 0, 0]) and np.array_equal(out[1], [255, 255, 255]), (matrix, order)
        m, oy, oc = _coefficients(matrix, "limited", order, depth)
        out = pf.convert_yuv(e(16 * s, 235 * s), e(128 * s, 128 * s), e(128 * s, 128 * s), m, oy, oc, shift)
        assert np.array_equal(out[0], [0, 0, 0]) and np.array_equal(out[1], [255, 255, 255]), (matrix, order)
    # a code >= 0x8000 is unsigned, and a 10-bit code lands on a quarter step of the 0 .. 255 scale, not on a whole one
    m, oy, oc = np.eye(3, dtype=np.float32) * np.float32(1.0 / s), np.float32(0), np.float32(0)
    half = 1 << (depth - 1)                                         # (the element 0x8000)
    out = pf.convert_yuv(e(half), e(5), e(half + 1), m, oy, oc, shift)
    assert np.array_equal(out[0], [128, 5.0 / s, 128 + 1.0 / s]) and (depth == 16 or out[0, 1] != round(out[0, 1]))


def test_the_restatement_is_pinned_on_the_recorded_case():
    """d = 10: all 1024 luma codes with an 8 x 8 grid of (U, V) (pf.combinations10, one 256 x 256 frame); d = 12 and 16: pf.extremes.
    The SHA-256 of the restatement's float32 output for each matrix / range / order, and the output itself for the first four rows of
    the d = 10 frame under bt2020 / limited / bgr."""
    y, uv = pf.combinations10()
    assert sorted(set((y >> 6).ravel().tolist())) == list(range(1024))
    assert {0, 512, 1023} <= set((uv >> 6).ravel().tolist()) and len({tuple(p) for p in (uv >> 6).reshape(-1, 2).tolist()}) == 64
    seen = {(int(a), int(u), int(v)) for a, (u, v) in zip((y >> 6)[0].ravel(), np.repeat(np.repeat(uv[0] >> 6, 2, 0), 2, 1).reshape(-1, 2))}
    assert len(seen) == 1024 * 64
    recorded = dict(l.rsplit(" ", 1) for l in open(os.path.join(GOLDEN, "p010_convert_sha256.txt")).read().strip().split("\n"))
    assert len(recorded) == 36
    for depth in pf.DEPTHS:
        py, pu = (y, uv) if depth == 10 else pf.extremes(depth)
        for v in pf.VARIANTS:
            m, oy, oc = _coefficients(*v, depth)
            out = pf.convert(py, pu, m, oy, oc, 16 - depth)
            assert out.dtype == np.float32 and out.min() >= 0 and out.max() <= 255
            assert pf.digest(out) == recorded["%d %s" % (depth, " ".join(v))], (depth, v)
    rows = np.load(os.path.join(GOLDEN, "p010_convert_bt2020_limited_bgr_rows0_3.npy"))
    m, oy, oc = _coefficients("bt2020", "limited", "bgr", 10)
    out = pf.convert(y, uv, m, oy, oc, 6)
    assert np.array_equal(out[0, :4].view(np.uint32), rows.view(np.uint32))
    # not rounded to integers, and the clamp acts
    assert np.any(rows != np.round(rows)) and np.any(rows == 0) and np.any(out == 255)


# ----------------------------------------------------------------------------- what the frames can see

N, H, W = 2, 24, 34
DEPTH = 10


@pytest.fixture(scope="module")
def correct_pyramid():
    y, uv = pf.batch(N, H, W, DEPTH)
    m, oy, oc = _coefficients("bt709", "limited", "bgr", DEPTH)
    frames = pf.convert(y, uv, m, oy, oc, 16 - DEPTH)
    return (y, uv, m, oy, oc), frames, [so.classic_pyramid(f, 2.0, 2) for f in frames]


def _beyond_assert_close(got, want, what):
    """True when conftest.assert_close, with the rounding bound of the zoom, refuses ``got`` for ``want`` on some level."""
    for l, (g, w) in enumerate(zip(got, want)):
        try:
            assert_close(g.astype(np.float32), w, 1e-5, scale=255.0, what="%s level %d" % (what, l), bound=eb.zoom(w))
        except AssertionError:
            return True
    return False


def test_the_surfaces_carry_the_batch_under_both_fills(correct_pyramid):
    (y, uv, m, oy, oc), frames, want = correct_pyramid
    yr, yf, ur, uf = pf.layout(N, H, W)[:4]
    assert yr != ur and yf != H * yr and uf != (H // 2) * ur and pf.layout(N, H, W)[5] % 2 == 1
    assert len(pf.MISTAKES) == 13 and {"the shift dropped", "oc = 128 instead of 128 s", "the element loaded signed", "V one byte after U",
                                       "byte strides taken as element strides"} <= set(pf.MISTAKES)
    for fill in pf.FILLS:
        py, pu = pf.place(y, uv, fill)
        seen = pf.truth(py, pu, N, H, W, m, oy, oc, 16 - DEPTH)
        assert np.array_equal(seen.view(np.uint32), frames.view(np.uint32))
        my, mu = pf.pixel_mask(N, H, W)
        assert np.all(py[~my] == fill * 0x0101) and np.all(pu[~mu] == fill * 0x0101) and my.sum() == N * H * W and mu.sum() == N * H * W // 2
        assert not _beyond_assert_close(so.classic_pyramid(seen[1], 2.0, 2), want[1], "truth")


@pytest.mark.parametrize("name", sorted(pf.MISTAKES))
def test_the_surfaces_separate_each_mistake_from_the_truth(correct_pyramid, name):
    """The oracle's pyramid of what a mistaken loader would see differs from the true one by more than assert_close allows, under at
    least one of the two fills, on every frame where the mistake acts (frame 1 for the frame stride)."""
    (y, uv, m, oy, oc), frames, want = correct_pyramid
    shown = False
    for fill in pf.FILLS:
        py, pu = pf.place(y, uv, fill)
        seen = pf.MISTAKES[name](py, pu, N, H, W, m, oy, oc, 16 - DEPTH)
        assert seen.shape == frames.shape and seen.dtype == np.float32
        shown = shown or all(_beyond_assert_close(so.classic_pyramid(seen[f], 2.0, 2), want[f], name) for f in pf.FRAMES_HIT.get(name, (0, 1)))
    assert shown, "%s is invisible on these frames" % name


# ----------------------------------------------------------------------------- the host side under the sanitizers

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@needs_hipcc
def test_p010_entry_points_on_the_host_side_under_asan_and_ubsan():
    """Both forms of both entry points on 40 x 58 surfaces whose planes are heap blocks of exactly their spans, for a classic and a crop
    plan; the staged bytes are the two spans and the poisoned arena behind them is untouched; the status codes and the order of the
    checks.  No sanitizer report, one "ok" line."""
    from test_gray_uint8_host import run_driver
    assert "rgb p010 host main ok" in run_driver("rgb_p010")


@needs_hipcc
def test_every_single_fault_of_the_p010_forms_is_refused_with_the_recorded_status_and_message():
    from test_gray_uint8_host import run_driver
    got = run_driver("rgb_p010", "--refusals").strip().split("\n")
    want = open(os.path.join(GOLDEN, "p010_refusals.txt")).read().strip().split("\n")
    assert len(want) == 2 * 27 + 2 * 24 and {l.split(" | ")[0] for l in want} == set(NAMES)
    assert got == want
    for l in want:
        name, case, status, text = l.split(" | ")
        assert text.startswith(name.replace("_dev", "") + ": "), l
        assert status == ("-4" if case == "single-channel plan" else "-1"), l
    single = [l for l in want if "single-channel plan" in l]
    assert len(single) == 2 and all("silent_pyramid_view16)" in l for l in single)
    assert sum("even H and W" in l for l in want) == 8 and sum("must be finite" in l for l in want) == 12
    assert sum("2-byte aligned" in l for l in want) == 8 and sum("stride is odd" in l for l in want) == 16 and sum("shift must be" in l for l in want) == 8
    # the order of the cases in the table is the order of the checks: NV12's, then address, stride, shift, then the shared ones
    cases = [l.split(" | ")[1] for l in want if l.startswith("silent_pyramid_p010 |")]
    assert cases.index("oc not finite") < cases.index("y address odd") < cases.index("y_row_stride odd") < cases.index("shift -1") < cases.index("out NULL")


def _address_plans():
    from pysilent_amd.util.zoom.from_image import classic_levels
    from test_rgb_nv12_host import odd_origin_crops
    return [((40, 8), classic_levels((40, 8), 2.0, 2)), ((64, 66), classic_levels((64, 66), 2.0, 3)),
            ((134, 242), classic_levels((134, 242), 2.0, 4)), odd_origin_crops()[::2]]


@needs_hipcc
@pytest.mark.parametrize("which", range(4), ids=["classic-40x8", "classic-64x66", "classic-134x242", "crops-270x482"])
def test_every_address_of_the_walk_loader_lies_inside_its_span_and_covers_the_crops(which):
    """--addresses: w3_p010_load -- the function pyramid_walk3_kernel forms its P010 loads with -- for every block, chunk, row, lane and
    load slot of the plan's launch on two frames: no access (2 luma bytes, 4 chroma bytes) outside the luma span or the chroma span,
    every offset even, the luma element of every crop pixel and the pair under it among the bytes touched, no byte touched that is not
    a pixel's."""
    from test_gray_uint8_host import run_driver
    hw, levels = _address_plans()[which]
    out = run_driver("rgb_p010", "--addresses", str(hw[0]), str(hw[1]), str(len(levels)), *[str(int(v)) for l in levels for v in l])
    lines = [l for l in out.strip().split("\n") if l]
    assert len(lines) == 1, out
    f = lines[0].split(" | ")
    assert f[0] == "%d x %d" % hw and f[3] == "outside 0" and f[4].endswith("missing y 0 uv 0") and f[5] == "not a pixel byte 0", lines[0]
    assert f[7] == "unaligned 0", lines[0]
    assert int(f[4].split()[1]) > 0 and int(f[2].split()[1]) > 0, lines[0]
    if which == 3:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
        assert "plans 2 " in f[1] and int(f[6].split()[2]) >= 1, lines[0]
