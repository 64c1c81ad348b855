"""16-bit planar, semi-planar and packed YUV for 3-channel plans on the GPU (silent_yuv16_to_rgb[_dev], silent_pyramid_yuv16[_dev],
PyramidPlan.run(rgb_frame_format="yuv420p10" ...), LineEndPipeline(mode="rgb", rgb_frame_format=...)): the conversion equals the
NumPy restatement of tests/rgb_yuv16_frames.py BIT FOR BIT on every layout, and the pyramid is that of silent_pyramid on the
restatement's float32 frames bit for bit -- host form and _dev form, on every route of launch_pyramid3 (the walk kernel, union and
per-level plans, the border pixels inside and behind the walk's launch, the unit + region kernels) -- and with it every map and keypoint
of the RGB pipeline.  The planes lie in parents whose bytes are 0x00 and then 0xFF, with random bits outside the code
(tests/test_rgb_yuv16_host.py shows what they can see)."""
import ctypes as C
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_p010_frames as pf
import rgb_yuv16_frames as wf
import rgb_yuv_frames as yf
import silent_oracle as so
from conftest import assert_close
from test_rgb_nv12_host import odd_origin_crops
from test_rgb_uint8 import _outputs, _same, _same_outputs, _t

pytestmark = pytest.mark.gpu
E5 = math.e ** .5
DEFAULT = ("bt709", "limited", "bgr")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _kw(variant):
    return dict(nv12_matrix=variant[0], nv12_range=variant[1], nv12_order=variant[2])


def _triples(s, Y, U, V, fill):
    """(the parents, host (y, u, v) views, device (y, u, v) views) of the batch in parents whose bytes are ``fill``."""
    parents = wf.place(s, Y, U, V, fill)
    dev = wf.torch_views(s, [_t(p).cuda(0) for p in parents])
    return parents, wf.views(s, parents), dev


def _hw_of(name, hw, odd):
    """The extents a layout is converted on: odd where the subsampling allows it (4:2:2: odd H; 4:4:4: odd H and W)."""
    s = wf.LAYOUTS[name](1, 4, 4)
    return (hw[0] + (odd and not s["sy"]), hw[1] - (odd and not s["sx"]))


class _Struct(object):
    """silent_yuv16_to_rgb[_dev] / silent_pyramid_yuv16[_dev] called with the struct built by hand (the C level: 4:4:0 and the depths
    9 and 14 have no rgb_frame_format)."""

    def __init__(self, rt):
        import torch
        from pysilent_amd import _lib
        self.rt, self.torch, self._lib, self.lib, self.ctx = rt, torch, _lib, _lib.load(), rt.get_context(0)

    def to_rgb(self, s, parents, m, oy, oc, dev):
        torch = self.torch
        n, H, W = s["n"], s["H"], s["W"]
        if dev:
            keep = [_t(p).cuda(0) for p in parents]
            out = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda:0")
            ptr = self._lib.yuv16_ptr(wf.struct_args(s, [k.data_ptr() for k in keep], m, oy, oc))
            self.ctx.check(self.lib.silent_yuv16_to_rgb_dev(self.ctx.handle, ptr, n, H, W, C.c_void_p(out.data_ptr()),
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            return out
        out = np.empty((n, H, W, 3), np.float32)
        ptr = self._lib.yuv16_ptr(wf.struct_args(s, [p.ctypes.data for p in parents], m, oy, oc))
        self.ctx.check(self.lib.silent_yuv16_to_rgb(self.ctx.handle, ptr, n, H, W, out.ctypes.data_as(C.c_void_p)))
        return out

    def pyramid(self, plan, s, parents, m, oy, oc):
        torch = self.torch
        keep = [_t(p).cuda(0) for p in parents]
        out = torch.empty(s["n"] * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
        ptr = self._lib.yuv16_ptr(wf.struct_args(s, [k.data_ptr() for k in keep], m, oy, oc))
        self.ctx.check(self.lib.silent_pyramid_yuv16_dev(self.ctx.handle, plan.handle, ptr, s["n"], C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return out


# ----------------------------------------------------------------------------- the conversion

CONVERSIONS = [(name, odd) for name in wf.LAYOUTS for odd in (False, True) if not odd or wf.LAYOUTS[name](1, 4, 4)["sub"] in ("422", "444")]


@pytest.mark.parametrize("name,odd", CONVERSIONS, ids=["%s%s" % (n, "-odd" if o else "") for n, o in CONVERSIONS])
def test_conversion_equals_the_restatement_bit_for_bit(rt, name, odd):
    """silent_yuv16_to_rgb_dev and the host form on every layout under both fills: 2 x 24 x 34 frames, and 2 x 25 x 34 for 4:2:2 and
    2 x 25 x 33 for 4:4:4.  Depth 10 on every layout family, 12 and 16 on i0xx / p2xx / y2xx / y416; depth 9 (low bits), depth 14 (bits
    1 .. 14) and 4:4:0 through the struct built by hand, the others through _runtime.yuv16_to_rgb as well."""
    H, W = _hw_of(name, (24, 34), odd)
    assert (H, W) in ((24, 34), (25, 34), (25, 33))
    s = wf.spec(name, 2, H, W)
    Y, U, V = wf.batch(s, seed=1)
    m, oy, oc = wf.coefficients(*DEFAULT, depth=s["depth"])
    c = _Struct(rt)
    for fill in wf.FILLS:
        parents, host, dev = _triples(s, Y, U, V, fill)
        want = wf.truth(s, parents, m, oy, oc)
        for form in (True, False):
            _same(c.to_rgb(s, parents, m, oy, oc, form), want, "%s %dx%d, fill 0x%02X, struct, %s form" % (name, H, W, fill, "_dev" if form else "host"))
        if name in wf.PYTHON_LAYOUTS:
            got = rt.yuv16_to_rgb(dev, (H, W), s["fmt"])
            assert got.is_cuda and tuple(got.shape) == (2, H, W, 3)
            _same(got, want, "%s, fill 0x%02X, _dev form" % (name, fill))
            _same(rt.yuv16_to_rgb(host, (H, W), s["fmt"]), want, "%s, fill 0x%02X, host form" % (name, fill))


@pytest.mark.parametrize("variant", pf.VARIANTS, ids=["-".join(v) for v in pf.VARIANTS])
def test_conversion_variants(rt, variant):
    """The twelve matrix / range / order variants (bt2020 among them) on the Y210 and the I012 layout under both fills."""
    for name in ("y210", "i012"):
        s = wf.spec(name, 2, 24, 34)
        m, oy, oc = wf.coefficients(*variant, depth=s["depth"])
        Y, U, V = wf.batch(s, seed=2)
        for fill in wf.FILLS:
            parents, host, dev = _triples(s, Y, U, V, fill)
            want = wf.truth(s, parents, m, oy, oc)
            _same(rt.yuv16_to_rgb(dev, (24, 34), s["fmt"], *variant), want, "%s %s, fill 0x%02X, _dev form" % (name, variant, fill))
            _same(rt.yuv16_to_rgb(host, (24, 34), s["fmt"], *variant), want, "%s %s, fill 0x%02X, host form" % (name, variant, fill))


def test_conversion_with_a_matrix_of_the_callers(rt):
    """A 3 x 3 array is on the 8-bit scale, as for P010: multiplied by 2^-(depth - 8); nv12_range gives oy."""
    m = np.array([[.5, -1.25, 2.0], [1.0, 0.0, 0.0], [-.75, .3, .1]], np.float32)
    s = wf.spec("i010", 2, 24, 34)
    parents, _, dev = _triples(s, *wf.batch(s, seed=3), 0xFF)
    _same(rt.yuv16_to_rgb(dev, (24, 34), "yuv420p10", m, "full"), wf.truth(s, parents, m * np.float32(.25), 0.0, 512.0), "a 3 x 3 array, full range")
    _same(rt.yuv16_to_rgb(dev, (24, 34), "yuv420p10", m.tolist(), "limited"), wf.truth(s, parents, m * np.float32(.25), 64.0, 512.0),
          "a 3 x 3 list, limited range")


# ----------------------------------------------------------------------------- pyramids

def _check_planes(rt, plan, name, n, hw, what, knobs=(0, 2), variant=DEFAULT, seed=0):
    """_dev form and host form under both fills and each PYRAMID knob against silent_pyramid on the restatement's float32 frames."""
    from pysilent_amd._lib import TUNE_PYRAMID
    s = wf.spec(name, n, hw[0], hw[1])
    m, oy, oc = wf.coefficients(*variant, depth=s["depth"])
    Y, U, V = wf.batch(s, seed=seed)
    f32 = _t(wf.truth(s, wf.place(s, Y, U, V, 0), m, oy, oc)).cuda(0)
    kw = dict(rgb_frame_format=s["fmt"], **_kw(variant))
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            got = []
            for fill in wf.FILLS:
                _, host, dev = _triples(s, Y, U, V, fill)
                tag = "%s %s, fill 0x%02X, PYRAMID knob %d" % (name, what, fill, knob)
                got_dev, got_host = plan.run(dev, **kw), plan.run(host, **kw)
                assert got_dev.on_device and not got_host.on_device and got_dev.channels == got_host.channels == 3
                _same(got_dev, want, tag + ", _dev form")
                _same(got_host, want, tag + ", host form")
                got.append(got_dev)
            _same(got[0], got[1], "%s %s, PYRAMID knob %d: the two fills" % (name, what, knob))


CLASSIC = [((40, 8), 2.0, 2, (1, 36)),                # one strip, W below a strip
           ((64, 66), 2.0, 3, (1, 36)),               # W % 4 != 0
           ((136, 240), 2.0, 4, (1, 36)),             # W % 4 == 0, several strips and segments
           ((134, 242), 2.0, 4, (1, 36)),
           ((40, 8), E5, 2, None), ((64, 66), E5, 3, None), ((136, 240), E5, 4, None), ((134, 242), E5, 4, None)]
FULL = ("i010", "y210")
# the full list for I010 and Y210; (64, 66) and (134, 242) for every other layout; (65, 66) for 4:2:2 and (41, 9) for 4:4:4
CLASSIC_CASES = [(name, c) for name in FULL for c in CLASSIC]
CLASSIC_CASES += [(name, c) for name in wf.PYTHON_LAYOUTS if name not in FULL for c in CLASSIC if c[0] in ((64, 66), (134, 242))]
CLASSIC_CASES += [(name, ((65, 66), sc, 3, None)) for name in ("i210", "y210") for sc in (2.0, E5)]
CLASSIC_CASES += [(name, ((41, 9), sc, 2, None)) for name in ("i410", "y416") for sc in (2.0, E5)]


@pytest.mark.parametrize("name,case", CLASSIC_CASES, ids=["%s-%dx%d-s%.3g-n%d" % ((n,) + c[0] + c[1:3]) for n, c in CLASSIC_CASES])
def test_classic_pyramids_bit_identical_to_the_float32_call(rt, name, case):
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n, route = case
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    assert plan.walk_plans[0] == 1 and plan.walk_plans[1] in (24, 28, 32, 36) and (route is None or plan.walk_plans == route), plan.walk_plans
    for frames in (1, 3):
        _check_planes(rt, plan, name, frames, hw, "classic %s scale %.3g n %d, %d frames" % (hw, scale, n, frames), seed=n)
    plan.close()


def _crops():
    hw, center, _ = odd_origin_crops()
    return [((480, 640), (288, 192), E5), (hw, center, 2.0)]


@pytest.mark.parametrize("name", ("i010", "p210", "y210"))
@pytest.mark.parametrize("which", range(2), ids=["reference-480x640", "odd-origin-270x482"])
def test_crop_layouts_bit_identical_to_the_float32_call(rt, which, name):
    """The union plan with its border pixels inside the walk's launch (knob 0) and behind it (knob 8), the unit + region kernels
    (knob 2), and one plan per level (knob 4 at plan creation).  The second layout's innermost crop starts at an odd row and an odd
    column: (x0 + x) >> 1 is not x0 / 2 + x / 2 there."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import reference_levels
    hw, center, scale = _crops()[which]
    levels = reference_levels(hw, center, scale)
    if which == 1:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
    plan = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert plan.walk_plans[0] == (2 if len(levels) >= 3 else len(levels)), plan.walk_plans
    _check_planes(rt, plan, name, 2, hw, "crops %s" % (hw,), knobs=(0, 2, 8), seed=len(levels))
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert per_level.walk_plans[0] == len(levels)
    _check_planes(rt, per_level, name, 2, hw, "crops %s, one plan per level" % (hw,), knobs=(0, 8), seed=len(levels))
    plan.close()
    per_level.close()


@pytest.mark.parametrize("name", ("yuv440", "i009", "m014"))
def test_the_c_level_structs(rt, name):
    """4:4:0, depth 9 in the low bits and depth 14 in bits 1 .. 14 have no rgb_frame_format: silent_pyramid_yuv16_dev with the struct
    built by hand, against silent_pyramid on the restatement's frames, walk kernel and unit + region kernels."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 67) if name == "yuv440" else (64, 66)
    s = wf.spec(name, 2, hw[0], hw[1])
    Y, U, V = wf.batch(s, seed=4)
    m, oy, oc = wf.coefficients(*DEFAULT, depth=s["depth"])
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    c = _Struct(rt)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            for fill in wf.FILLS:
                parents = wf.place(s, Y, U, V, fill)
                want = plan.run(_t(wf.truth(s, parents, m, oy, oc)).cuda(0))
                _same(c.pyramid(plan, s, parents, m, oy, oc), want.data, "%s, fill 0x%02X, PYRAMID knob %d" % (name, fill, knob))
    plan.close()


def test_a_triple_into_p010_surfaces_gives_the_p010_bits(rt):
    """A 4:2:0 triple pointing into P010 surfaces (v == u + 1 element, shift == 16 - depth: the P010 kernels' dispatch) gives exactly
    plan.run(..., rgb_frame_format="p010")'s bits; the same picture as I010 (codes >> 6, low-aligned) and as a VU-swapped semi-planar
    triple (the general kernels) gives them too; so does yuv16_to_rgb against p010_to_rgb."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, n = (134, 242), 2
    y, uv = pf.batch(n, hw[0], hw[1], 10, seed=6)
    U, V = np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])
    py, pu = pf.place(y, uv, 0xFF)
    dy, du = _t(py).cuda(0), _t(pu).cuda(0)
    p010_pair = pf.torch_views(dy, du, n, hw[0], hw[1])
    s = wf.spec("p010", n, hw[0], hw[1])
    triple = wf.torch_views(s, [dy, du])
    assert triple[2].data_ptr() == triple[1].data_ptr() + 2 == p010_pair[1].data_ptr() + 2 and triple[1].stride(2) == 2
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 4))
    others = {"vu010": ("yuv420p10msb", _triples(wf.spec("vu010", n, hw[0], hw[1]), y, U, V, 0x00)[2]),
              "i010": ("yuv420p10", _triples(wf.spec("i010", n, hw[0], hw[1]), y >> 6, U >> 6, V >> 6, 0xFF)[2])}
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(p010_pair, rgb_frame_format="p010")
            _same(plan.run(triple, rgb_frame_format="yuv420p10msb"), want, "a triple into P010 surfaces, PYRAMID knob %d" % knob)
            for name, (fmt, t) in others.items():
                _same(plan.run(t, rgb_frame_format=fmt), want, "the same picture as %s, PYRAMID knob %d" % (name, knob))
    want = rt.p010_to_rgb(p010_pair, hw, 10)
    _same(rt.yuv16_to_rgb(triple, hw, "yuv420p10msb"), want, "conversion of a triple into P010 surfaces")
    for name, (fmt, t) in others.items():
        _same(rt.yuv16_to_rgb(t, hw, fmt), want, "conversion of the same picture as %s" % name)
    plan.close()


def test_widened_bytes_give_the_8_bit_yuv420_pyramid(rt):
    """byte << 2 low-aligned and (byte << 8) | garbage high-aligned triples with limited-range coefficients give the pyramid
    rgb_frame_format="yuv420" gives for the bytes, bit for bit."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, n = (64, 66), 2
    s8 = yf.spec("i420", n, hw[0], hw[1])
    B = yf.batch(s8, seed=8)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    want = plan.run(tuple(_t(b).cuda(0) for b in B), rgb_frame_format="yuv420")
    rng = np.random.default_rng(3)
    low = tuple(b.astype(np.uint16) << 2 for b in B)
    high = tuple((b.astype(np.uint16) << 8) | rng.integers(0, 64, b.shape).astype(np.uint16) for b in B)
    _same(plan.run(_triples(wf.spec("i010", n, hw[0], hw[1]), *low, 0xFF)[2], rgb_frame_format="yuv420p10"), want, "byte << 2, low-aligned")
    _same(plan.run(_triples(wf.spec("vu010", n, hw[0], hw[1]), *high, 0xFF)[2], rgb_frame_format="yuv420p10msb"), want, "(byte << 8) | garbage")
    plan.close()


def test_against_the_oracle_on_the_converted_frame(rt):
    """Directly, not through the float32 path: so.classic_pyramid of the restatement's frame, within the zoom's rounding bound."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (136, 240), 2.0, 4
    s = wf.spec("y210", 2, hw[0], hw[1])
    Y, U, V = wf.batch(s, seed=n)
    m, oy, oc = wf.coefficients(*DEFAULT, depth=10)
    parents, _, dev = _triples(s, Y, U, V, 0xFF)
    frames = wf.truth(s, parents, m, oy, oc)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(dev, rgb_frame_format="yuv422p10msb")
    for f in range(2):
        want = so.classic_pyramid(frames[f], scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="y210 frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


def test_chroma_offsets_past_2_31(rt):
    """Two 64 x 66 frames whose CHROMA planes lie 2^31 + 4098 bytes apart inside one uninitialised 2.2 GiB allocation (_dev form), the
    luma planes packed: frame 1's chroma addresses need the 64-bit frame term on every route -- a 32-bit one would read in front of the
    plane."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 66)
    ch, cw = hw[0] // 2, hw[1] // 2
    stride, row = ((1 << 31) + 4098) // 2, cw + 6             # elements
    plane = (ch - 1) * row + cw
    span = stride + 2 * plane + 64
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * span + (1 << 28):
        pytest.skip("not enough free device memory for a 2.2 GiB allocation")
    big = torch.empty(span + 16, dtype=torch.uint16, device="cuda:0")
    u_view = torch.as_strided(big, (2, ch, cw), (stride, row, 1), 3)
    v_view = torch.as_strided(big, (2, ch, cw), (stride, row, 1), 3 + plane + 11)
    s = wf.spec("i010", 2, hw[0], hw[1])
    Y, U, V = wf.batch(s, seed=3)
    assert not np.array_equal(U[0], U[1]) and not np.array_equal(V[0], V[1])
    u_view.copy_(_t(U).cuda(0))
    v_view.copy_(_t(V).cuda(0))
    dy = _t(Y).cuda(0)
    assert u_view[1].data_ptr() - u_view[0].data_ptr() == (1 << 31) + 4098 == v_view[1].data_ptr() - v_view[0].data_ptr()
    m, oy, oc = wf.coefficients(*DEFAULT, depth=10)
    f32 = _t(wf.convert(Y, U, V, 1, 1, m, oy, oc, 0, 10)).cuda(0)
    _same(rt.yuv16_to_rgb((dy, u_view, v_view), hw, "yuv420p10"), f32, "c_frame_stride 2^31 + 4098, conversion")
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same(plan.run((dy, u_view, v_view), rgb_frame_format="yuv420p10"), plan.run(f32), "c_frame_stride 2^31 + 4098, PYRAMID knob %d" % knob)
    plan.close()
    del u_view, v_view, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals

def test_refusals_of_the_wrapper(rt):
    """The planes pass as they are; the C entry point's own refusals arrive as ValueError with its text -- every line of
    tests/golden/yuv16_refusals.txt that can be provoked through the struct from Python (a plan of another context: the host program)."""
    import torch
    from pysilent_amd import _lib
    s = wf.spec("i012", 2, 40, 48)
    Y, U, V = wf.batch(s)
    dy, du, dv = _t(Y).cuda(0), _t(U).cuda(0), _t(V).cuda(0)
    FMT = dict(rgb_frame_format="yuv420p12")
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    wide = torch.zeros((2, 20, 48), dtype=torch.uint16, device="cuda:0")
    for bad, text in (((dy.to(torch.float32), du, dv), "uint16"), ((dy.to(torch.uint8), du, dv), "uint16"), ((dy, du[:1], dv), "chroma planes"),
                      ((dy[:, :38], du, dv), "luma plane"), ((dy, U, V), "must either be"), ((dy, du), "triple"), (dy, "triple"),
                      ((dy, du, wide[:, :, ::2]), "u and v must have equal strides")):
        with pytest.raises((ValueError, TypeError), match=text):
            plan.run(bad, **FMT)
    with pytest.raises(ValueError, match="chroma planes"):
        plan.run((dy, du, dv), rgb_frame_format="yuv444p12")
    with pytest.raises(ValueError, match="rgb_frame_format='yuv420p12' does not combine with rgb_frame_dtype='uint8'"):
        plan.run((dy, du, dv), rgb_frame_dtype="uint8", **FMT)
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_format='yuv420p12' is for mode 'rgb'"):
        gray.run((dy, du, dv), **FMT)
    odd = rt.PyramidPlan(40, 47, 3, [(0, 0, 40, 47, 40, 47, 40, 47)])
    with pytest.raises(ValueError, match="needs even H and W"):
        odd.run((dy, du, dv), **FMT)
    lib, ctx = _lib.load(), plan.ctx
    out = torch.empty(2 * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
    optr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, oy, oc = wf.coefficients(*DEFAULT, depth=12)
    good = rt.yuv16_frames_of((dy, du, dv), (40, 48), "yuv420p12", m, oy, oc)[0]
    assert good[3:11] == (2, 96, 40 * 96, 2, 48, 20 * 48, 1, 1) and good[14:] == (0, 12)

    def call(handle, frames, n, pyr=optr):
        ctx.check(lib.silent_pyramid_yuv16_dev(ctx.handle, handle, _lib.yuv16_ptr(frames), n, pyr, stream))

    def put(i, v, *more):
        t = good[:i] + (v,) + good[i + 1:]
        return put_in(t, *more) if more else t

    def put_in(t, i, v, *more):
        t = t[:i] + (v,) + t[i + 1:]
        return put_in(t, *more) if more else t

    nan9 = [float("nan")] * 9
    call(plan.handle, good, 2)
    P = "silent_pyramid_yuv16: "
    for args, text in (((None, good, 2), P + "NULL pointer"), ((plan.handle, None, 2), P + "NULL pointer"),
                       ((plan.handle, put(0, 0), 2), P + "NULL pointer"), ((plan.handle, put(1, 0), 2), P + "NULL pointer"),
                       ((plan.handle, put(2, 0), 2), P + "NULL pointer"),
                       ((plan.handle, put(9, 2), 2), P + "a chroma shift must be 0 or 1"),
                       ((plan.handle, put(10, -1), 2), P + "a chroma shift must be 0 or 1"),
                       ((odd.handle, good, 2), P + "a subsampled axis needs an even extent"),
                       ((plan.handle, put(3, 1), 2), P + "a pixel stride is below 2"),
                       ((plan.handle, put(6, -2), 2), P + "a pixel stride is below 2"),
                       ((plan.handle, put(4, 94), 2), P + "y_row_stride is below"),
                       ((plan.handle, put(7, 46), 2), P + "c_row_stride is below"),
                       ((plan.handle, put(5, 40 * 96 - 2), 2), P + "y_frame_stride is below"),
                       ((plan.handle, put(5, 0), 2), P + "y_frame_stride is below"),
                       ((plan.handle, put(8, 20 * 48 - 2), 2), P + "c_frame_stride is below"),
                       ((plan.handle, put(8, 1 << 62), 3), P + r"a plane spans more than 2\^63 bytes"),
                       ((plan.handle, put(11, nan9), 2), P + "m, oy and oc must be finite"),
                       ((plan.handle, put(12, float("inf")), 2), P + "m, oy and oc must be finite"),
                       ((plan.handle, put(13, float("-inf")), 2), P + "m, oy and oc must be finite"),
                       ((plan.handle, put(0, good[0] + 1), 2), P + "y, u and v must be 2-byte aligned"),
                       ((plan.handle, put(1, good[1] + 1), 2), P + "y, u and v must be 2-byte aligned"),
                       ((plan.handle, put(2, good[2] + 1), 2), P + "y, u and v must be 2-byte aligned"),
                       ((plan.handle, put(3, 3, 4, 200, 5, 40 * 200), 2), P + "a stride is odd"),
                       ((plan.handle, put(7, 49, 8, 20 * 50), 2), P + "a stride is odd"),
                       ((plan.handle, put(8, 20 * 48 + 1), 2), P + "a stride is odd"),
                       ((plan.handle, put(15, 7), 2), P + "depth must be 8 .. 16"), ((plan.handle, put(15, 17), 2), P + "depth must be 8 .. 16"),
                       ((plan.handle, put(14, -1), 2), P + "shift must be 0 .. 16 - depth"),
                       ((plan.handle, put(14, 5), 2), P + "shift must be 0 .. 16 - depth"),
                       ((plan.handle, good, 2, None), P + "NULL pointer"),
                       ((plan.handle, good, 0), P + "n_frames must be >= 1"),
                       ((gray.handle, good, 2), r"single-channel plan reads the luma plane through silent_pyramid_view16\)")):
        with pytest.raises(ValueError, match=text):
            call(*args)
    rgb = torch.empty((2, 40, 48, 3), dtype=torch.float32, device="cuda:0")
    for frames, n, h, w, ptr, text in ((put(15, 7), 2, 40, 48, rgb.data_ptr(), "silent_yuv16_to_rgb: depth must be 8 .. 16"),
                                       (good, 2, 41, 48, rgb.data_ptr(), "silent_yuv16_to_rgb: a subsampled axis needs an even extent"),
                                       (good, 0, 40, 48, rgb.data_ptr(), "silent_yuv16_to_rgb: n_frames must be >= 1"),
                                       (good, 2, 40, 48, None, "silent_yuv16_to_rgb: NULL pointer")):
        with pytest.raises(ValueError, match=text):
            ctx.check(lib.silent_yuv16_to_rgb_dev(ctx.handle, _lib.yuv16_ptr(frames), n, h, w, C.c_void_p(ptr), stream))
    torch.cuda.synchronize()
    for p in (plan, gray, odd):
        p.close()


# ----------------------------------------------------------------------------- the pipeline

PIPES = [((136, 240), dict(n_levels=4, scale=2.0)), ((480, 640), dict(center_dimensions=(288, 192), scale=E5))]
# one name per subsampling and alignment class
PIPE_LAYOUTS = {"yuv420p10": "i010", "yuv422p10msb": "y210", "yuv444p12": "i412", "yuv420p10msb": "vu010", "yuv422p16": "p216",
                "yuv444p10msb": "p410", "yuv422p10": "i210", "yuv444p16": "y416", "yuv420p12": "i012"}


@pytest.mark.parametrize("fmt", sorted(PIPE_LAYOUTS))
@pytest.mark.parametrize("hw,geometry", PIPES, ids=["classic-136x240", "reference-480x640"])
def test_pipeline_yuv16_triples(rt, hw, geometry, fmt):
    """LineEndPipeline(mode="rgb", rgb_frame_format=fmt, selection=True): step((y, u, v)) reads the planes in place; pyramid, orient,
    line_end, keypoints and counts equal the float32 pipeline's on the restatement's frames (which are yuv16_to_rgb's, bit for bit)
    under both fills; step_host gives the same on packed and on strided host planes."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    batch, name = 2, PIPE_LAYOUTS[fmt]
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **geometry)
    s = wf.spec(name, batch, hw[0], hw[1])
    assert s["fmt"] == fmt
    m, oy, oc = wf.coefficients(*DEFAULT, depth=s["depth"])
    batches = [wf.batch(s, seed=11), wf.batch(s, seed=12)]
    ref = LineEndPipeline(hw, **kw)
    want = []
    for b in batches:
        frames = rt.yuv16_to_rgb(_triples(s, *b, 0)[2], hw, fmt)
        _same(frames, wf.truth(s, wf.place(s, *b, 0), m, oy, oc), "yuv16_to_rgb of the batch")
        ref.step(frames)
        want.append(_outputs(ref))
    assert {n for n, _ in want[0]} >= {"pyramid", "orient", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(want[0], want[1]) if a.shape == b.shape)

    pipe = LineEndPipeline(hw, rgb_frame_format=fmt, **kw)
    assert pipe.rgb_frame_format == fmt and pipe.rgb_frame_dtype == "float32" and pipe.frame_dtype == "float32"
    assert "%s read in place" % fmt.upper() in pipe.launch_summary() and pipe.launch_summary().startswith(ref.launch_summary())
    px = hw[0] * hw[1] if pipe.crop_px is None else pipe.crop_px
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 12 * px + px * {"420": 3, "422": 4, "444": 6}[s["sub"]]
    for fill in wf.FILLS:
        for i, b in enumerate(batches):
            pipe.step(_triples(s, *b, fill)[2])
            _same_outputs(_outputs(pipe), want[i], "step, fill 0x%02X, batch %d" % (fill, i))
    for i in (0, 1, 0):
        pipe.step_host(batches[i])
        _same_outputs(_outputs(pipe), want[i], "step_host, batch %d" % i)
    pipe.step_host(wf.views(s, wf.place(s, *batches[1], 0xFF)))
    _same_outputs(_outputs(pipe), want[1], "step_host on strided host planes")
    for bad, text in (((batches[0][0].astype(np.float32),) + tuple(batches[0][1:]), "triple of uint16 arrays"), (batches[0][0], "triple of uint16 arrays")):
        with pytest.raises(ValueError, match=text):
            pipe.step_host(bad)
    dev = _triples(s, *batches[0], 0)[2]
    for bad, text in (((dev[0].to(torch.float32),) + tuple(dev[1:]), "uint16"), (tuple(p[:1] for p in dev), "triple"), (dev[0], "triple")):
        with pytest.raises(ValueError, match=text):
            pipe.step(bad)
    synth = pipe._synthetic_frames()
    assert [tuple(p.shape) for p in synth] == [tuple(p.shape) for p in batches[0]] and all(p.dtype == torch.uint16 and p.is_cuda for p in synth)
    for p in (ref, pipe):
        p.close()


def test_pipeline_surfaces_and_other_coefficients(rt):
    """nv12_matrix / nv12_range / nv12_order reach the kernels: bt2020 / full / rgb against the float32 pipeline on that conversion;
    the planes are cut out of pitched P210 surfaces by util.zoom.yuv16_planes."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom import yuv16_planes, YUV16_LAYOUTS
    hw, variant = (136, 240), ("bt2020", "full", "rgb")
    kw = dict(mode="rgb", batch=2, device=0, selection=True, placement=None, n_levels=4, scale=2.0)
    s = wf.spec("p210", 2, hw[0], hw[1])
    Y, U, V = wf.batch(s, seed=5)
    m, oy, oc = wf.coefficients(*variant, depth=10)
    surf = torch.full((2, 2 * hw[0], 1024), 0xA5A5, dtype=torch.uint16, device="cuda:0")
    planes = yuv16_planes(surf, hw[0], hw[1], "p210")
    assert YUV16_LAYOUTS["p210"] == "yuv422p10msb" == s["fmt"] and planes[2].data_ptr() == planes[1].data_ptr() + 2
    for p, data in zip(planes, (Y, U, V)):
        p.copy_(_t(data).cuda(0))
    ref, pipe = LineEndPipeline(hw, **kw), LineEndPipeline(hw, rgb_frame_format="yuv422p10msb", **dict(kw, **_kw(variant)))
    ref.step(_t(wf.convert(Y, U, V, 1, 0, m, oy, oc, 6, 10)).cuda(0))
    pipe.step(planes)
    _same_outputs(_outputs(pipe), _outputs(ref), "bt2020 / full / rgb on yuv16_planes of P210 surfaces")
    for p in (ref, pipe):
        p.close()
