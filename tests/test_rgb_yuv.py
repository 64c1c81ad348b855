"""Planar and packed 8-bit YUV for 3-channel plans on the GPU (silent_yuv_to_rgb[_dev], silent_pyramid_yuv[_dev],
PyramidPlan.run(rgb_frame_format="yuv420" / "yuv422" / "yuv444"), LineEndPipeline(mode="rgb", rgb_frame_format=...)): the conversion
equals the NumPy restatement of tests/rgb_yuv_frames.py BIT FOR BIT on every layout, and the pyramid is that of silent_pyramid on the
restatement's float32 frames bit for bit -- host form and _dev form, on every route of launch_pyramid3 (the walk kernel, union and
per-level plans, the border pixels inside and behind the walk's launch, the unit + region kernels) -- and with it every map and keypoint
of the RGB pipeline.  The planes lie in parents filled with 0x00 and then with 0xFF (tests/test_rgb_yuv_host.py shows what they can
see)."""
import ctypes as C
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
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
    """(the parents, host (y, u, v) views, device (y, u, v) views) of the batch in parents filled with ``fill``."""
    parents = yf.place(s, Y, U, V, fill)
    dev = yf.torch_views(s, [_t(p).cuda(0) for p in parents])
    return parents, yf.views(s, parents), dev


def _hw_of(name, hw, odd):
    """The extents a layout is converted on: odd where the format allows it (4:2:2: odd H; 4:4:4: odd H and W)."""
    sx, sy = yf.LAYOUTS[name](1, 4, 4)["sx"], yf.LAYOUTS[name](1, 4, 4)["sy"]
    return (hw[0] + (odd and not sy), hw[1] - (odd and not sx))


# ----------------------------------------------------------------------------- the conversion

class _Struct(object):
    """silent_yuv_to_rgb[_dev] / silent_pyramid_yuv[_dev] called with the struct built by hand (the C level: 4:4:0 has no
    rgb_frame_format)."""

    def __init__(self, rt):
        import torch
        from pysilent_amd import _lib
        self.rt, self.torch, self._lib, self.lib, self.ctx = rt, torch, _lib, _lib.load(), rt.get_context(0)

    def to_rgb(self, s, parents, m, oy, dev):
        torch = self.torch
        n, H, W = s["n"], s["H"], s["W"]
        if dev:
            keep = [_t(p).cuda(0) for p in parents]
            out = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda:0")
            ptr = self._lib.yuv_ptr(yf.struct_args(s, [k.data_ptr() for k in keep], m, oy))
            self.ctx.check(self.lib.silent_yuv_to_rgb_dev(self.ctx.handle, ptr, n, H, W, C.c_void_p(out.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            return out
        out = np.empty((n, H, W, 3), np.float32)
        ptr = self._lib.yuv_ptr(yf.struct_args(s, [p.ctypes.data for p in parents], m, oy))
        self.ctx.check(self.lib.silent_yuv_to_rgb(self.ctx.handle, ptr, n, H, W, out.ctypes.data_as(C.c_void_p)))
        return out

    def pyramid(self, plan, s, parents, m, oy):
        torch = self.torch
        keep = [_t(p).cuda(0) for p in parents]
        out = torch.empty(s["n"] * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
        ptr = self._lib.yuv_ptr(yf.struct_args(s, [k.data_ptr() for k in keep], m, oy))
        self.ctx.check(self.lib.silent_pyramid_yuv_dev(self.ctx.handle, plan.handle, ptr, s["n"], C.c_void_p(out.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return out


CONVERSIONS = [(name, odd) for name in yf.LAYOUTS for odd in (False, True)
               if not odd or name in ("i422", "nv16", "yuyv", "uyvy", "i444", "vuya")]


@pytest.mark.parametrize("name,odd", CONVERSIONS, ids=["%s%s" % (n, "-odd" if o else "") for n, o in CONVERSIONS])
def test_conversion_equals_the_restatement_bit_for_bit(rt, name, odd):
    """silent_yuv_to_rgb_dev and the host form on every layout under both fills: 2 x 24 x 34 frames, and 2 x 25 x 34 for 4:2:2 and
    2 x 25 x 33 for 4:4:4 (odd extents where the format allows them).  Through the struct for every layout (4:4:0 has no
    rgb_frame_format) and through _runtime.yuv_to_rgb for those with one."""
    H, W = _hw_of(name, (24, 34), odd)
    assert (H, W) in ((24, 34), (25, 34), (25, 33))
    s = yf.spec(name, 2, H, W)
    Y, U, V = yf.batch(s, seed=1)
    m, oy = nf.coefficients(*DEFAULT)
    c = _Struct(rt)
    for fill in yf.FILLS:
        parents, host, dev = _triples(s, Y, U, V, fill)
        want = yf.truth(s, parents, m, oy)
        for form in (True, False):
            _same(c.to_rgb(s, parents, m, oy, form), want, "%s %dx%d, fill 0x%02X, struct, %s form" % (name, H, W, fill, "_dev" if form else "host"))
        if name in yf.PYTHON_LAYOUTS:
            got = rt.yuv_to_rgb(dev, (H, W), s["fmt"])
            assert got.is_cuda and tuple(got.shape) == (2, H, W, 3)
            _same(got, want, "%s, fill 0x%02X, _dev form" % (name, fill))
            _same(rt.yuv_to_rgb(host, (H, W), s["fmt"]), want, "%s, fill 0x%02X, host form" % (name, fill))


@pytest.mark.parametrize("variant", nf.VARIANTS, ids=["-".join(v) for v in nf.VARIANTS])
def test_conversion_variants_and_all_combinations(rt, variant):
    """The eight matrix / range / order variants on the YUYV layout under both fills, and on the frame that holds all 256 Y values with
    a 16 x 16 grid of (U, V) re-expressed as I420 (contiguous planes)."""
    m, oy = nf.coefficients(*variant)
    s = yf.spec("yuyv", 2, 24, 34)
    Y, U, V = yf.batch(s, seed=2)
    for fill in yf.FILLS:
        parents, host, dev = _triples(s, Y, U, V, fill)
        want = yf.truth(s, parents, m, oy)
        _same(rt.yuv_to_rgb(dev, (24, 34), "yuv422", *variant), want, "%s, fill 0x%02X, _dev form" % (variant, fill))
        _same(rt.yuv_to_rgb(host, (24, 34), "yuv422", *variant), want, "%s, fill 0x%02X, host form" % (variant, fill))
    y, uv = nf.combinations()
    u, v = np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])
    _same(rt.yuv_to_rgb((_t(y).cuda(0), _t(u).cuda(0), _t(v).cuda(0)), (256, 256), "yuv420", *variant), nf.convert(y, uv, m, oy),
          "%s, all combinations as I420" % (variant,))


def test_conversion_with_a_matrix_of_the_callers(rt):
    m = np.array([[.5, -1.25, 2.0], [1.0, 0.0, 0.0], [-.75, .3, .1]], np.float32)
    s = yf.spec("i420", 2, 24, 34)
    parents, _, dev = _triples(s, *yf.batch(s, seed=3), 0xFF)
    _same(rt.yuv_to_rgb(dev, (24, 34), "yuv420", m, "full"), yf.truth(s, parents, m, 0.0), "a 3 x 3 array, full range")
    _same(rt.yuv_to_rgb(dev, (24, 34), "yuv420", m.tolist(), "limited"), yf.truth(s, parents, m, 16.0), "a 3 x 3 list, limited range")


# ----------------------------------------------------------------------------- pyramids

def _check_planes(rt, plan, name, n, hw, what, knobs=(0, 2), variant=DEFAULT, seed=0):
    """_dev form and host form under both fills and each PYRAMID knob against silent_pyramid on the restatement's float32 frames."""
    from pysilent_amd._lib import TUNE_PYRAMID
    m, oy = nf.coefficients(*variant)
    s = yf.spec(name, n, hw[0], hw[1])
    Y, U, V = yf.batch(s, seed=seed)
    f32 = _t(yf.truth(s, yf.place(s, Y, U, V, 0), m, oy)).cuda(0)
    kw = dict(rgb_frame_format=s["fmt"], **_kw(variant))
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            got = []
            for fill in yf.FILLS:
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
FULL = ("i420", "yuyv")
# the full list for I420 and YUYV; (64, 66) and (134, 242) for every other layout; (65, 66) for 4:2:2 and (41, 9) for 4:4:4
CLASSIC_CASES = [(name, c) for name in FULL for c in CLASSIC]
CLASSIC_CASES += [(name, c) for name in yf.PYTHON_LAYOUTS if name not in FULL for c in CLASSIC if c[0] in ((64, 66), (134, 242))]
CLASSIC_CASES += [(name, ((65, 66), sc, 3, None)) for name in ("i422", "yuyv") for sc in (2.0, E5)]
CLASSIC_CASES += [(name, ((41, 9), sc, 2, None)) for name in ("i444", "vuya") for sc in (2.0, E5)]


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


@pytest.mark.parametrize("name", ("i420", "nv21", "yuyv"))
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


def test_the_440_struct_on_the_c_level(rt):
    """chroma_shift_x = 0, chroma_shift_y = 1 has no rgb_frame_format: silent_pyramid_yuv_dev with the struct built by hand, against
    silent_pyramid on the restatement's frames, walk kernel and unit + region kernels."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 67)
    s = yf.spec("yuv440", 2, hw[0], hw[1])
    Y, U, V = yf.batch(s, seed=4)
    m, oy = nf.coefficients(*DEFAULT)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    c = _Struct(rt)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            for fill in yf.FILLS:
                parents = yf.place(s, Y, U, V, fill)
                want = plan.run(_t(yf.truth(s, parents, m, oy)).cuda(0))
                _same(c.pyramid(plan, s, parents, m, oy), want.data, "4:4:0, fill 0x%02X, PYRAMID knob %d" % (fill, knob))
    plan.close()


def test_a_420_triple_into_nv12_surfaces_gives_the_nv12_bits(rt):
    """A 4:2:0 triple pointing into NV12 surfaces (v == u + 1: the NV12 kernels' dispatch) gives exactly
    plan.run(..., rgb_frame_format="nv12")'s bits; the same picture as NV21 and as I420 (the general kernels) gives them too."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, n = (134, 242), 2
    y, uv = nf.batch(n, hw[0], hw[1], seed=6)
    U, V = np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])
    py, pu = nf.place(y, uv, 0xFF)
    dy, du = _t(py).cuda(0), _t(pu).cuda(0)
    nv12_pair = nf.torch_views(dy, du, n, hw[0], hw[1])
    s = yf.spec("nv12", n, hw[0], hw[1])
    triple = yf.torch_views(s, [dy, du])
    assert triple[2].data_ptr() == triple[1].data_ptr() + 1 == nv12_pair[1].data_ptr() + 1 and triple[1].stride(2) == 2
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 4))
    others = {}
    for name in ("nv21", "i420"):
        so_ = yf.spec(name, n, hw[0], hw[1])
        others[name] = _triples(so_, y, U, V, 0x00)[2]
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(nv12_pair, rgb_frame_format="nv12")
            _same(plan.run(triple, rgb_frame_format="yuv420"), want, "a triple into NV12 surfaces, PYRAMID knob %d" % knob)
            for name, t in others.items():
                _same(plan.run(t, rgb_frame_format="yuv420"), want, "the same picture as %s, PYRAMID knob %d" % (name, knob))
    _same(rt.yuv_to_rgb(triple, hw, "yuv420"), rt.nv12_to_rgb(nv12_pair, hw), "conversion of a triple into NV12 surfaces")
    plan.close()


def test_against_the_oracle_on_the_converted_frame(rt):
    """Directly, not through the float32 path: so.classic_pyramid of the restatement's frame, within the zoom's rounding bound (the
    statement of test_rgb_nv12.test_against_the_oracle_on_the_converted_frame)."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (136, 240), 2.0, 4
    s = yf.spec("yuyv", 2, hw[0], hw[1])
    Y, U, V = yf.batch(s, seed=n)
    m, oy = nf.coefficients(*DEFAULT)
    parents, _, dev = _triples(s, Y, U, V, 0xFF)
    frames = yf.truth(s, parents, m, oy)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(dev, rgb_frame_format="yuv422")
    for f in range(2):
        want = so.classic_pyramid(frames[f], scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="yuyv frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


def test_chroma_offsets_past_2_31(rt):
    """Two 64 x 66 frames whose CHROMA planes lie 2^31 + 4099 bytes apart inside one uninitialised 2.2 GiB allocation (_dev form), the
    luma planes packed: frame 1's chroma addresses need the 64-bit frame term on every route -- a 32-bit one would read frame 0's."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 66)
    ch, cw = hw[0] // 2, hw[1] // 2
    stride, row = (1 << 31) + 4099, cw + 6
    plane = (ch - 1) * row + cw
    span = stride + 2 * plane + 64
    free, _ = torch.cuda.mem_get_info(0)
    if free < span + (1 << 28):
        pytest.skip("not enough free device memory for a 2.2 GiB allocation")
    big = torch.empty(span + 16, dtype=torch.uint8, device="cuda:0")
    u_view = torch.as_strided(big, (2, ch, cw), (stride, row, 1), 3)
    v_view = torch.as_strided(big, (2, ch, cw), (stride, row, 1), 3 + plane + 11)
    s = yf.spec("yv12", 2, hw[0], hw[1])
    Y, U, V = yf.batch(s, seed=3)
    assert not np.array_equal(U[0], U[1]) and not np.array_equal(V[0], V[1])
    u_view.copy_(_t(U).cuda(0))
    v_view.copy_(_t(V).cuda(0))
    dy = _t(Y).cuda(0)
    assert u_view[1].data_ptr() - u_view[0].data_ptr() == stride == v_view[1].data_ptr() - v_view[0].data_ptr()
    m, oy = nf.coefficients(*DEFAULT)
    yy, xx = np.arange(hw[0])[:, None] >> 1, np.arange(hw[1])[None, :] >> 1
    f32 = _t(nf.convert_yuv(Y, U[:, yy, xx], V[:, yy, xx], m, oy)).cuda(0)
    _same(rt.yuv_to_rgb((dy, u_view, v_view), hw, "yuv420"), f32, "c_frame_stride 2^31 + 4099, conversion")
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same(plan.run((dy, u_view, v_view), rgb_frame_format="yuv420"), plan.run(f32), "c_frame_stride 2^31 + 4099, PYRAMID knob %d" % knob)
    plan.close()
    del u_view, v_view, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals

def test_refusals_of_the_wrapper(rt):
    """The planes pass as they are; the C entry point's own refusals arrive as ValueError with its text."""
    import torch
    from pysilent_amd import _lib
    s = yf.spec("yv12", 2, 40, 48)
    Y, U, V = yf.batch(s)
    dy, du, dv = _t(Y).cuda(0), _t(U).cuda(0), _t(V).cuda(0)
    YUV = dict(rgb_frame_format="yuv420")
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    wide = torch.zeros((2, 20, 48), dtype=torch.uint8, device="cuda:0")
    for bad, text in (((dy.to(torch.float32), du, dv), "uint8"), ((dy, du[:1], dv), "chroma planes"), ((dy[:, :38], du, dv), "luma plane"),
                      ((dy, U, V), "must either be"), ((dy, du), "triple"), (dy, "triple"),
                      ((dy, du, wide[:, :, ::2]), "u and v must have equal strides")):
        with pytest.raises((ValueError, TypeError), match=text):
            plan.run(bad, **YUV)
    with pytest.raises(ValueError, match="chroma planes"):
        plan.run((dy, du, dv), rgb_frame_format="yuv444")
    with pytest.raises(ValueError, match="rgb_frame_format='yuv420' does not combine with rgb_frame_dtype='uint8'"):
        plan.run((dy, du, dv), rgb_frame_dtype="uint8", **YUV)
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_format='yuv420' is for mode 'rgb'"):
        gray.run((dy, du, dv), **YUV)
    odd = rt.PyramidPlan(40, 47, 3, [(0, 0, 40, 47, 40, 47, 40, 47)])
    with pytest.raises(ValueError, match="needs even H and W"):
        odd.run((dy, du, dv), **YUV)
    lib, ctx = _lib.load(), plan.ctx
    out = torch.empty(2 * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
    optr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, oy = nf.coefficients(*DEFAULT)
    good = rt.yuv_frames_of((dy, du, dv), (40, 48), "yuv420", m, oy)[0]
    assert good[3:11] == (1, 48, 40 * 48, 1, 24, 20 * 24, 1, 1)

    def call(handle, frames, n, pyr=optr):
        ctx.check(lib.silent_pyramid_yuv_dev(ctx.handle, handle, _lib.yuv_ptr(frames), n, pyr, stream))

    def put(i, v):
        return good[:i] + (v,) + good[i + 1:]

    call(plan.handle, good, 2)
    for args, text in (((plan.handle, put(9, 2), 2), "silent_pyramid_yuv: a chroma shift must be 0 or 1"),
                       ((plan.handle, put(3, 0), 2), "silent_pyramid_yuv: a pixel stride is below 1"),
                       ((plan.handle, put(4, 47), 2), "silent_pyramid_yuv: y_row_stride is below"),
                       ((plan.handle, put(7, 23), 2), "silent_pyramid_yuv: c_row_stride is below"),
                       ((plan.handle, put(8, 479), 2), "silent_pyramid_yuv: c_frame_stride is below"),
                       ((plan.handle, put(11, [float("nan")] * 9), 2), "silent_pyramid_yuv: m and oy must be finite"),
                       ((odd.handle, good, 2), "silent_pyramid_yuv: a subsampled axis needs an even extent"),
                       ((plan.handle, good, 0), "silent_pyramid_yuv: n_frames must be >= 1"),
                       ((plan.handle, good, 2, None), "silent_pyramid_yuv: NULL pointer"),
                       ((gray.handle, good, 2), r"single-channel plan reads the luma plane through silent_pyramid_view\)")):
        with pytest.raises(ValueError, match=text):
            call(*args)
    torch.cuda.synchronize()
    for p in (plan, gray, odd):
        p.close()


# ----------------------------------------------------------------------------- the pipeline

PIPES = [((136, 240), dict(n_levels=4, scale=2.0)), ((480, 640), dict(center_dimensions=(288, 192), scale=E5))]
PIPE_LAYOUTS = {"yuv420": "i420", "yuv422": "yuyv", "yuv444": "i444"}


@pytest.mark.parametrize("fmt", sorted(PIPE_LAYOUTS))
@pytest.mark.parametrize("hw,geometry", PIPES, ids=["classic-136x240", "reference-480x640"])
def test_pipeline_yuv_triples(rt, hw, geometry, fmt):
    """LineEndPipeline(mode="rgb", rgb_frame_format=fmt, selection=True): step((y, u, v)) reads the planes in place; pyramid, orient,
    line_end, keypoints and counts equal the float32 pipeline's on the restatement's frames bit for bit, under both fills; step_host
    gives the same (packed and strided host planes); overlap="force" gives the same; yuv_planes on surfaces gives the same as
    explicit planes."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom import yuv_planes
    batch, name = 2, PIPE_LAYOUTS[fmt]
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **geometry)
    m, oy = nf.coefficients(*DEFAULT)
    s = yf.spec(name, batch, hw[0], hw[1])
    batches = [yf.batch(s, seed=11), yf.batch(s, seed=12)]
    ref = LineEndPipeline(hw, **kw)
    want = []
    for b in batches:
        ref.step(_t(yf.truth(s, yf.place(s, *b, 0), m, oy)).cuda(0))
        want.append(_outputs(ref))
    assert {n for n, _ in want[0]} >= {"pyramid", "orient", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(want[0], want[1]) if a.shape == b.shape)

    pipe = LineEndPipeline(hw, rgb_frame_format=fmt, **kw)
    assert pipe.rgb_frame_format == fmt and pipe.rgb_frame_dtype == "float32" and pipe.frame_dtype == "float32"
    assert "%s read in place" % fmt.upper() in pipe.launch_summary() and pipe.launch_summary().startswith(ref.launch_summary())
    px = hw[0] * hw[1] if pipe.crop_px is None else pipe.crop_px
    per_px = {"yuv420": (3, 2), "yuv422": (2, 1), "yuv444": (3, 1)}[fmt]
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 12 * px + px * per_px[0] // per_px[1]
    for fill in yf.FILLS:
        for i, b in enumerate(batches):
            pipe.step(_triples(s, *b, fill)[2])
            _same_outputs(_outputs(pipe), want[i], "step, fill 0x%02X, batch %d" % (fill, i))
    pipe.step(tuple(_t(p).cuda(0) for p in batches[1]))
    _same_outputs(_outputs(pipe), want[1], "step on contiguous planes")
    for i in (0, 1, 0):
        pipe.step_host(batches[i])
        _same_outputs(_outputs(pipe), want[i], "step_host, batch %d" % i)
    pipe.step_host(yf.views(s, yf.place(s, *batches[1], 0xFF)))
    _same_outputs(_outputs(pipe), want[1], "step_host on strided host planes")
    # surfaces as a source delivers them: yuv_planes cuts the triple out, nothing copied
    rows, pitch = {"i420": (hw[0] * 3 // 2, 2048), "yuyv": (hw[0], 2048), "i444": (3 * hw[0], 1024)}[name]
    surf = torch.full((batch, rows, pitch), 0xA5, dtype=torch.uint8, device="cuda:0")
    planes = yuv_planes(surf, hw[0], hw[1], name)
    assert all(p.data_ptr() >= surf.data_ptr() and p.data_ptr() < surf.data_ptr() + surf.numel() for p in planes)
    for p, data in zip(planes, batches[0]):
        p.copy_(_t(data).cuda(0))
    pipe.step(planes)
    _same_outputs(_outputs(pipe), want[0], "step on yuv_planes of pitched surfaces")
    for bad, text in (((planes[0].to(torch.float32),) + tuple(planes[1:]), "uint8"), (tuple(p[:1] for p in planes), "triple"), (planes[0], "triple")):
        with pytest.raises(ValueError, match=text):
            pipe.step(bad)
    with pytest.raises(ValueError, match="triple of uint8 arrays"):
        pipe.step_host(batches[0][0])
    over = LineEndPipeline(hw, rgb_frame_format=fmt, overlap="force", **kw)
    for i in (0, 1):
        over.step(_triples(s, *batches[i], 0xFF)[2])
        _same_outputs(_outputs(over), want[i], "overlap='force', batch %d" % i)
    # the tuners' synthetic frames are a triple of the format's shapes, and a tuned pipeline computes the same
    synth = pipe._synthetic_frames()
    assert [tuple(p.shape) for p in synth] == [tuple(p.shape) for p in batches[0]] and all(p.dtype == torch.uint8 and p.is_cuda for p in synth)
    tuned = LineEndPipeline(hw, rgb_frame_format=fmt, **kw)
    assert tuned.tune_placement(tries=2, steps=2, budget_s=0.3)["stopped_by"] in ("tries", "budget_s", "memory cap", "allocation failed")
    tuned.step(_triples(s, *batches[1], 0x00)[2])
    _same_outputs(_outputs(tuned), want[1], "after the placement tuner on its own synthetic triple")
    for p in (ref, pipe, over, tuned):
        p.close()


def test_pipeline_other_coefficients(rt):
    """nv12_matrix / nv12_range / nv12_order reach the kernels: bt601 / full / rgb against the float32 pipeline on that conversion."""
    from pysilent_amd.pipeline import LineEndPipeline
    hw, variant = (136, 240), ("bt601", "full", "rgb")
    kw = dict(mode="rgb", batch=2, device=0, selection=True, placement=None, n_levels=4, scale=2.0)
    s = yf.spec("yuyv", 2, hw[0], hw[1])
    Y, U, V = yf.batch(s, seed=5)
    m, oy = nf.coefficients(*variant)
    parents, _, dev = _triples(s, Y, U, V, 0x00)
    ref, pipe = LineEndPipeline(hw, **kw), LineEndPipeline(hw, rgb_frame_format="yuv422", **dict(kw, **_kw(variant)))
    ref.step(_t(yf.truth(s, parents, m, oy)).cuda(0))
    pipe.step(dev)
    _same_outputs(_outputs(pipe), _outputs(ref), "bt601 / full / rgb")
    for p in (ref, pipe):
        p.close()
