"""NV12 decoder surfaces for 3-channel plans on the GPU (silent_nv12_to_rgb[_dev], silent_pyramid_nv12[_dev],
PyramidPlan.run(rgb_frame_format="nv12"), LineEndPipeline(mode="rgb", rgb_frame_format="nv12")): the conversion equals the NumPy
restatement of tests/rgb_nv12_frames.py BIT FOR BIT, and the pyramid is that of silent_pyramid on the restatement's float32 frames
bit for bit -- host form and _dev form, on every route of launch_pyramid3 (the walk kernel, union and per-level plans, the border
pixels inside and behind the walk's launch, the unit + region kernels) -- and with it every map and keypoint of the RGB pipeline.
The planes lie in two parents with different pitches, filled with 0x00 and then with 0xFF (tests/test_rgb_nv12_host.py shows what
they can see)."""
import ctypes as C
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
import silent_oracle as so
from conftest import assert_close
from test_rgb_nv12_host import odd_origin_crops
from test_rgb_uint8 import _outputs, _same, _same_outputs, _t

pytestmark = pytest.mark.gpu
NV12 = dict(rgb_frame_format="nv12")
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


def _surfaces(y, uv, fill):
    """(host (y, uv) views, device (y, uv) views) of the planes in parents filled with ``fill`` (nf.layout: two pitches, gaps)."""
    n, H, W = y.shape
    py, pu = nf.place(y, uv, fill)
    host = nf.views(py, pu, n, H, W)
    dev = nf.torch_views(_t(py).cuda(0), _t(pu).cuda(0), n, H, W)
    assert not dev[0].is_contiguous() and not dev[1].is_contiguous() and dev[1].data_ptr() % 2 == 1
    return host, dev


# ----------------------------------------------------------------------------- the conversion

@pytest.mark.parametrize("variant", nf.VARIANTS, ids=["-".join(v) for v in nf.VARIANTS])
def test_conversion_equals_the_restatement_bit_for_bit(rt, variant):
    """silent_nv12_to_rgb_dev and the host form on pitched 2 x 24 x 34 surfaces under both fills, and on the frame that holds all 256 Y
    values with a 16 x 16 grid of (U, V) (contiguous planes)."""
    m, oy = nf.coefficients(*variant)
    y, uv = nf.batch(2, 24, 34, seed=1)
    want = nf.convert(y, uv, m, oy)
    for fill in nf.FILLS:
        host, dev = _surfaces(y, uv, fill)
        got = rt.nv12_to_rgb(dev, (24, 34), *variant)
        assert got.is_cuda and tuple(got.shape) == (2, 24, 34, 3)
        _same(got, want, "%s, fill 0x%02X, _dev form" % (variant, fill))
        _same(rt.nv12_to_rgb(host, (24, 34), *variant), want, "%s, fill 0x%02X, host form" % (variant, fill))
    y, uv = nf.combinations()
    _same(rt.nv12_to_rgb((_t(y).cuda(0), _t(uv).cuda(0)), (256, 256), *variant), nf.convert(y, uv, m, oy), "%s, all combinations" % (variant,))


def test_conversion_with_a_matrix_of_the_callers(rt):
    m = np.array([[.5, -1.25, 2.0], [1.0, 0.0, 0.0], [-.75, .3, .1]], np.float32)
    y, uv = nf.batch(2, 24, 34, seed=2)
    _, dev = _surfaces(y, uv, 0xFF)
    _same(rt.nv12_to_rgb(dev, (24, 34), m, "full"), nf.convert(y, uv, m, 0.0), "a 3 x 3 array, full range")
    _same(rt.nv12_to_rgb(dev, (24, 34), m.tolist(), "limited"), nf.convert(y, uv, m, 16.0), "a 3 x 3 list, limited range")


# ----------------------------------------------------------------------------- pyramids

def _check_planes(rt, plan, y, uv, what, knobs=(0, 2), variant=DEFAULT):
    """_dev form and host form under both fills and each PYRAMID knob against silent_pyramid on the restatement's float32 frames."""
    from pysilent_amd._lib import TUNE_PYRAMID
    m, oy = nf.coefficients(*variant)
    f32 = _t(nf.convert(y, uv, m, oy)).cuda(0)
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            got = []
            for fill in nf.FILLS:
                host, dev = _surfaces(y, uv, fill)
                tag = "%s, fill 0x%02X, PYRAMID knob %d" % (what, fill, knob)
                got_dev, got_host = plan.run(dev, **dict(NV12, **_kw(variant))), plan.run(host, **dict(NV12, **_kw(variant)))
                assert got_dev.on_device and not got_host.on_device and got_dev.channels == got_host.channels == 3
                _same(got_dev, want, tag + ", _dev form")
                _same(got_host, want, tag + ", host form")
                got.append(got_dev)
            _same(got[0], got[1], "%s, PYRAMID knob %d: the two fills" % (what, knob))


CLASSIC = [((40, 8), 2.0, 2, (1, 36)),                # one strip, W below a strip
           ((64, 66), 2.0, 3, (1, 36)),               # W % 4 != 0
           ((136, 240), 2.0, 4, (1, 36)),             # W % 4 == 0, several strips and segments
           ((134, 242), 2.0, 4, (1, 36)),
           ((40, 8), E5, 2, None), ((64, 66), E5, 3, None), ((136, 240), E5, 4, None), ((134, 242), E5, 4, None)]


@pytest.mark.parametrize("hw,scale,n,route", CLASSIC, ids=["%dx%d-s%.3g-n%d" % (c[0] + c[1:3]) for c in CLASSIC])
def test_classic_pyramids_bit_identical_to_the_float32_call(rt, hw, scale, n, route):
    from pysilent_amd.util.zoom.from_image import classic_levels
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    assert plan.walk_plans[0] == 1 and plan.walk_plans[1] in (24, 28, 32, 36) and (route is None or plan.walk_plans == route), plan.walk_plans
    y, uv = nf.batch(3, hw[0], hw[1], seed=n)
    for frames in (1, 3):
        _check_planes(rt, plan, y[:frames], uv[:frames], "classic %s scale %.3g n %d, %d frames" % (hw, scale, n, frames))
    plan.close()


def _crops():
    hw, center, _ = odd_origin_crops()
    return [((480, 640), (288, 192), E5), (hw, center, 2.0)]


@pytest.mark.parametrize("which", range(2), ids=["reference-480x640", "odd-origin-270x482"])
def test_crop_layouts_bit_identical_to_the_float32_call(rt, which):
    """The union plan with its border pixels inside the walk's launch (knob 0) and behind it (knob 8), the unit + region kernels
    (knob 2), and one plan per level (knob 4 at plan creation).  The second layout's innermost crop starts at an odd row and an odd
    column: (x0 + x) >> 1 is not x0 / 2 + x / 2 there."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import reference_levels
    hw, center, scale = _crops()[which]
    levels = reference_levels(hw, center, scale)
    if which == 1:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
    y, uv = nf.batch(2, hw[0], hw[1], seed=len(levels))
    plan = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert plan.walk_plans[0] == (2 if len(levels) >= 3 else len(levels)), plan.walk_plans
    _check_planes(rt, plan, y, uv, "crops %s" % (hw,), knobs=(0, 2, 8))
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert per_level.walk_plans[0] == len(levels)
    _check_planes(rt, per_level, y, uv, "crops %s, one plan per level" % (hw,), knobs=(0, 8))
    plan.close()
    per_level.close()


def test_against_the_oracle_on_the_converted_frame(rt):
    """Directly, not through the float32 path: so.classic_pyramid of the restatement's frame, within the zoom's rounding bound (the
    statement of test_rgb_strided.test_against_the_oracle_on_the_widened_compacted_frame)."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (136, 240), 2.0, 4
    y, uv = nf.batch(2, hw[0], hw[1], seed=n)
    m, oy = nf.coefficients(*DEFAULT)
    frames = nf.convert(y, uv, m, oy)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(_surfaces(y, uv, 0xFF)[1], **NV12)
    for f in range(2):
        want = so.classic_pyramid(frames[f], scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="nv12 frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


def test_chroma_offsets_past_2_31(rt):
    """Two 64 x 66 frames whose CHROMA planes lie 2^31 + 4099 bytes apart inside one uninitialised 2.2 GiB allocation (_dev form), the
    luma planes packed: frame 1's chroma address needs the 64-bit frame term on every route -- a 32-bit one would read frame 0's."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 66)
    stride, row = (1 << 31) + 4099, hw[1] + 6
    span = stride + (hw[0] // 2 - 1) * row + hw[1]
    free, _ = torch.cuda.mem_get_info(0)
    if free < span + (1 << 28):
        pytest.skip("not enough free device memory for a 2.2 GiB allocation")
    big = torch.empty(span + 16, dtype=torch.uint8, device="cuda:0")
    uv_view = torch.as_strided(big, (2, hw[0] // 2, hw[1] // 2, 2), (stride, row, 2, 1), 3)
    y, uv = nf.batch(2, hw[0], hw[1], seed=3)
    assert not np.array_equal(uv[0], uv[1])
    uv_view.copy_(_t(uv).cuda(0))
    dy = _t(y).cuda(0)
    assert uv_view[1].data_ptr() - uv_view[0].data_ptr() == stride
    m, oy = nf.coefficients(*DEFAULT)
    f32 = _t(nf.convert(y, uv, m, oy)).cuda(0)
    _same(rt.nv12_to_rgb((dy, uv_view), hw), f32, "uv_frame_stride 2^31 + 4099, conversion")
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same(plan.run((dy, uv_view), **NV12), plan.run(f32), "uv_frame_stride 2^31 + 4099, PYRAMID knob %d" % knob)
    plan.close()
    del uv_view, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals

def test_refusals_of_the_wrapper(rt):
    """The planes pass as they are; the C entry point's own refusals arrive as ValueError with its text."""
    import torch
    from pysilent_amd import _lib
    y, uv = nf.batch(2, 40, 48)
    dy, du = _t(y).cuda(0), _t(uv).cuda(0)
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    for bad, text in (((dy.to(torch.float32), du), "uint8"), ((dy, du[:1]), "chroma plane"), ((dy[:, :38], du), "luma plane"),
                      ((dy, uv), "must either be"), (dy, "pair"),
                      ((dy, torch.as_strided(du, du.shape, (du.stride(0), du.stride(1), 1, 2))), "adjacent")):
        with pytest.raises((ValueError, TypeError), match=text):
            plan.run(bad, **NV12)
    with pytest.raises(ValueError, match="rgb_frame_format='nv12' does not combine with rgb_frame_dtype='uint8'"):
        plan.run((dy, du), rgb_frame_dtype="uint8", **NV12)
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_format='nv12' is for mode 'rgb'"):
        gray.run((dy, du), **NV12)
    odd = rt.PyramidPlan(40, 47, 3, [(0, 0, 40, 47, 40, 47, 40, 47)])
    with pytest.raises(ValueError, match="needs even H and W"):
        odd.run((dy, du), **NV12)
    lib, ctx = _lib.load(), plan.ctx
    out = torch.empty(2 * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
    optr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, oy = nf.coefficients(*DEFAULT)
    good = rt.nv12_frames_of((dy, du), (40, 48), m, oy)[0]

    def call(handle, frames, n, pyr=optr):
        ctx.check(lib.silent_pyramid_nv12_dev(ctx.handle, handle, _lib.nv12_ptr(frames), n, pyr, stream))

    call(plan.handle, good, 2)
    for args, text in (((plan.handle, good[:2] + (47,) + good[3:], 2), "silent_pyramid_nv12: y_row_stride is below W"),
                       ((plan.handle, good[:4] + (40,) + good[5:], 2), "silent_pyramid_nv12: uv_row_stride is below W"),
                       ((plan.handle, good[:5] + (900,) + good[6:], 2), "silent_pyramid_nv12: uv_frame_stride is below"),
                       ((plan.handle, good[:6] + ([float("nan")] * 9,) + good[7:], 2), "silent_pyramid_nv12: m and oy must be finite"),
                       ((odd.handle, good, 2), "silent_pyramid_nv12: NV12 frames need even H and W"),
                       ((plan.handle, good, 0), "silent_pyramid_nv12: n_frames must be >= 1"),
                       ((plan.handle, good, 2, None), "silent_pyramid_nv12: NULL pointer"),
                       ((gray.handle, good, 2), r"single-channel plan reads the luma plane through silent_pyramid_view\)")):
        with pytest.raises(ValueError, match=text):
            call(*args)
    torch.cuda.synchronize()
    for p in (plan, gray, odd):
        p.close()


# ----------------------------------------------------------------------------- the pipeline

PIPES = [((136, 240), dict(n_levels=4, scale=2.0)), ((480, 640), dict(center_dimensions=(288, 192), scale=E5))]


@pytest.mark.parametrize("hw,geometry", PIPES, ids=["classic-136x240", "reference-480x640"])
def test_pipeline_nv12_surfaces(rt, hw, geometry):
    """LineEndPipeline(mode="rgb", rgb_frame_format="nv12", selection=True): step((y, uv)) reads the planes in place; pyramid, orient,
    line_end and keypoints equal the float32 pipeline's on the restatement's frames bit for bit, under both fills; step_host gives the
    same; nv12_planes on [n, H * 3 / 2, 2048] surfaces gives the same as explicit planes."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom import nv12_planes
    batch = 2
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **geometry)
    y, uv = nf.batch(4, hw[0], hw[1], seed=11)
    m, oy = nf.coefficients(*DEFAULT)
    batches = [(y[0:2], uv[0:2]), (y[2:4], uv[2:4])]
    ref = LineEndPipeline(hw, **kw)
    want = []
    for b in batches:
        ref.step(_t(nf.convert(b[0], b[1], m, oy)).cuda(0))
        want.append(_outputs(ref))
    assert {n for n, _ in want[0]} >= {"pyramid", "orient", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(want[0], want[1]) if a.shape == b.shape)
    assert ref.rgb_frame_format == "interleaved" and "NV12" not in ref.launch_summary()

    pipe = LineEndPipeline(hw, rgb_frame_format="nv12", **kw)
    assert pipe.rgb_frame_format == "nv12" and pipe.rgb_frame_dtype == "float32" and pipe.frame_dtype == "float32"
    assert "NV12 read in place" in pipe.launch_summary() and pipe.launch_summary().startswith(ref.launch_summary())
    px = hw[0] * hw[1] if pipe.crop_px is None else pipe.crop_px
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 12 * px + px * 3 // 2
    assert pipe.pyramid_bytes_per_frame() == ref.pyramid_bytes_per_frame() - 12 * hw[0] * hw[1] + hw[0] * hw[1] * 3 // 2
    for fill in nf.FILLS:
        for i, b in enumerate(batches):
            pipe.step(_surfaces(b[0], b[1], fill)[1])
            _same_outputs(_outputs(pipe), want[i], "step, fill 0x%02X, batch %d" % (fill, i))
    pipe.step((_t(batches[1][0]).cuda(0), _t(batches[1][1]).cuda(0)))
    _same_outputs(_outputs(pipe), want[1], "step on contiguous planes")
    for i in (0, 1, 0):
        pipe.step_host(batches[i])
        _same_outputs(_outputs(pipe), want[i], "step_host, batch %d" % i)
    pipe.step_host(nf.views(*nf.place(batches[1][0], batches[1][1], 0xFF), batch, hw[0], hw[1]))
    _same_outputs(_outputs(pipe), want[1], "step_host on pitched host planes")
    # decoder surfaces: luma rows, chroma rows directly below, 2048-byte pitch
    surf = torch.full((batch, hw[0] * 3 // 2, 2048), 0xA5, dtype=torch.uint8, device="cuda:0")
    sy, su = nv12_planes(surf, hw[0], hw[1])
    assert sy.data_ptr() == surf.data_ptr() and su.data_ptr() == surf.data_ptr() + hw[0] * 2048 and su.stride() == (surf.stride(0), 2048, 2, 1)
    sy.copy_(_t(batches[0][0]).cuda(0))
    su.copy_(_t(batches[0][1]).cuda(0))
    pipe.step((sy, su))
    _same_outputs(_outputs(pipe), want[0], "step on nv12_planes of pitched surfaces")
    for bad, text in (((sy.to(torch.float32), su), "uint8"), ((sy[:1], su[:1]), "pair"), (sy, "pair")):
        with pytest.raises(ValueError, match=text):
            pipe.step(bad)
    with pytest.raises(ValueError, match="pair of uint8 arrays"):
        pipe.step_host(batches[0][0])
    with pytest.raises((ValueError, AttributeError, TypeError)):
        ref.step((sy, su))
    for p in (ref, pipe):
        p.close()


def test_pipeline_other_coefficients(rt):
    """nv12_matrix / nv12_range / nv12_order reach the kernels: bt601 / full / rgb against the float32 pipeline on that conversion."""
    from pysilent_amd.pipeline import LineEndPipeline
    hw, variant = (136, 240), ("bt601", "full", "rgb")
    kw = dict(mode="rgb", batch=2, device=0, selection=True, placement=None, n_levels=4, scale=2.0)
    y, uv = nf.batch(2, hw[0], hw[1], seed=5)
    m, oy = nf.coefficients(*variant)
    ref, pipe = LineEndPipeline(hw, **kw), LineEndPipeline(hw, rgb_frame_format="nv12", **dict(kw, **_kw(variant)))
    ref.step(_t(nf.convert(y, uv, m, oy)).cuda(0))
    pipe.step(_surfaces(y, uv, 0x00)[1])
    _same_outputs(_outputs(pipe), _outputs(ref), "bt601 / full / rgb")
    for p in (ref, pipe):
        p.close()
