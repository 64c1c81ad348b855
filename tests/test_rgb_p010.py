"""P010 / P012 / P016 decoder surfaces for 3-channel plans on the GPU (silent_p010_to_rgb[_dev], silent_pyramid_p010[_dev],
PyramidPlan.run(rgb_frame_format="p010"), LineEndPipeline(mode="rgb", rgb_frame_format="p010")): the conversion equals the NumPy
restatement of tests/rgb_p010_frames.py BIT FOR BIT, and the pyramid is that of silent_pyramid on the restatement's float32 frames
bit for bit -- host form and _dev form, on every route of launch_pyramid3 (the walk kernel, union and per-level plans, the border
pixels inside and behind the walk's launch, the unit + region kernels) -- and with it every map and keypoint of the RGB pipeline; on
(byte << 8) | junk surfaces it is the pyramid silent_pyramid_nv12 gives for the bytes.  The planes lie in two parents with different
pitches, the chroma plane at an address that is 2 (mod 4), the low bits of every element random, filled with 0x00 and then with 0xFF
(tests/test_rgb_p010_host.py shows what they can see)."""
import ctypes as C
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_nv12_frames as nf
import rgb_p010_frames as pf
import silent_oracle as so
from conftest import assert_close
from test_rgb_nv12 import CLASSIC, _crops
from test_rgb_uint8 import _outputs, _same, _same_outputs, _t

pytestmark = pytest.mark.gpu
P010 = dict(rgb_frame_format="p010")
FORMAT = {10: "p010", 12: "p012", 16: "p016"}
E5 = math.e ** .5
DEFAULT = ("bt709", "limited", "bgr")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _kw(variant, depth=10):
    return dict(rgb_frame_format=FORMAT[depth], nv12_matrix=variant[0], nv12_range=variant[1], nv12_order=variant[2])


def _surfaces(y, uv, fill):
    """(host (y, uv) views, device (y, uv) views) of the planes in parents filled with ``fill`` (pf.layout: two pitches, gaps, the
    chroma plane at 2 mod 4)."""
    n, H, W = y.shape
    py, pu = pf.place(y, uv, fill)
    host = pf.views(py, pu, n, H, W)
    dev = pf.torch_views(_t(py).cuda(0), _t(pu).cuda(0), n, H, W)
    assert not dev[0].is_contiguous() and not dev[1].is_contiguous() and dev[1].data_ptr() % 4 == 2 and dev[0].data_ptr() % 2 == 0
    return host, dev


def _dev(y, uv):
    return _t(y).cuda(0), _t(uv).cuda(0)


# ----------------------------------------------------------------------------- the conversion

@pytest.mark.parametrize("depth", pf.DEPTHS)
@pytest.mark.parametrize("variant", pf.VARIANTS, ids=["-".join(v) for v in pf.VARIANTS])
def test_conversion_equals_the_restatement_bit_for_bit(rt, variant, depth):
    """silent_p010_to_rgb_dev and the host form on pitched 2 x 24 x 34 surfaces with random low bits under both fills; for d = 10 on the
    frame that holds all 1024 luma codes with an 8 x 8 grid of (U, V), for d = 12 and 16 on the frame of extreme codes."""
    m, oy, oc = pf.coefficients(*variant, depth)
    y, uv = pf.batch(2, 24, 34, depth, seed=1)
    want = pf.convert(y, uv, m, oy, oc, 16 - depth)
    for fill in pf.FILLS:
        host, dev = _surfaces(y, uv, fill)
        got = rt.p010_to_rgb(dev, (24, 34), depth, *variant)
        assert got.is_cuda and tuple(got.shape) == (2, 24, 34, 3)
        _same(got, want, "%s d %d, fill 0x%02X, _dev form" % (variant, depth, fill))
        _same(rt.p010_to_rgb(host, (24, 34), depth, *variant), want, "%s d %d, fill 0x%02X, host form" % (variant, depth, fill))
    y, uv = pf.combinations10() if depth == 10 else pf.extremes(depth)
    _same(rt.p010_to_rgb(_dev(y, uv), y.shape[1:], depth, *variant), pf.convert(y, uv, m, oy, oc, 16 - depth),
          "%s d %d, all codes / extremes" % (variant, depth))


@pytest.mark.parametrize("depth", pf.DEPTHS)
def test_conversion_with_a_matrix_of_the_callers(rt, depth):
    """A 3 x 3 array is on the 8-bit scale: the library multiplies it by 2^-(d - 8) and takes oy from the range keyword."""
    m = np.array([[.5, -1.25, 2.0], [1.0, 0.0, 0.0], [-.75, .3, .1]], np.float32)
    s = np.float32(2.0 ** (depth - 8))
    y, uv = pf.batch(2, 24, 34, depth, seed=2)
    _, dev = _surfaces(y, uv, 0xFF)
    _same(rt.p010_to_rgb(dev, (24, 34), depth, m, "full"), pf.convert(y, uv, m / s, 0.0, 128 * s, 16 - depth), "a 3 x 3 array, full range")
    _same(rt.p010_to_rgb(dev, (24, 34), depth, m.tolist(), "limited"), pf.convert(y, uv, m / s, 16 * s, 128 * s, 16 - depth), "a 3 x 3 list, limited range")


# ----------------------------------------------------------------------------- pyramids

def _check_planes(rt, plan, y, uv, what, knobs=(0, 2), variant=DEFAULT, depth=10):
    """_dev form and host form under both fills and each PYRAMID knob against silent_pyramid on the restatement's float32 frames."""
    from pysilent_amd._lib import TUNE_PYRAMID
    m, oy, oc = pf.coefficients(*variant, depth)
    f32 = _t(pf.convert(y, uv, m, oy, oc, 16 - depth)).cuda(0)
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            got = []
            for fill in pf.FILLS:
                host, dev = _surfaces(y, uv, fill)
                tag = "%s, fill 0x%02X, PYRAMID knob %d" % (what, fill, knob)
                got_dev, got_host = plan.run(dev, **_kw(variant, depth)), plan.run(host, **_kw(variant, depth))
                assert got_dev.on_device and not got_host.on_device and got_dev.channels == got_host.channels == 3
                _same(got_dev, want, tag + ", _dev form")
                _same(got_host, want, tag + ", host form")
                got.append(got_dev)
            _same(got[0], got[1], "%s, PYRAMID knob %d: the two fills" % (what, knob))


@pytest.mark.parametrize("hw,scale,n,route", CLASSIC, ids=["%dx%d-s%.3g-n%d" % (c[0] + c[1:3]) for c in CLASSIC])
def test_classic_pyramids_bit_identical_to_the_float32_call(rt, hw, scale, n, route):
    """The eight classic cases of tests/test_rgb_nv12.py, with 1 and 3 frames."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    assert plan.walk_plans[0] == 1 and plan.walk_plans[1] in (24, 28, 32, 36) and (route is None or plan.walk_plans == route), plan.walk_plans
    y, uv = pf.batch(3, hw[0], hw[1], 10, seed=n)
    for frames in (1, 3):
        _check_planes(rt, plan, y[:frames], uv[:frames], "classic %s scale %.3g n %d, %d frames" % (hw, scale, n, frames))
    plan.close()


@pytest.mark.parametrize("which", range(2), ids=["reference-480x640", "odd-origin-270x482"])
def test_crop_layouts_bit_identical_to_the_float32_call(rt, which):
    """The two crop layouts of tests/test_rgb_nv12.py: the union plan with its border pixels inside the walk's launch (knob 0) and
    behind it (knob 8), the unit + region kernels (knob 2), and one plan per level (knob 4 at plan creation).  The second layout's
    innermost crop starts at an odd row and an odd column."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import reference_levels
    hw, center, scale = _crops()[which]
    levels = reference_levels(hw, center, scale)
    if which == 1:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
    y, uv = pf.batch(2, hw[0], hw[1], 10, seed=len(levels))
    plan = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert plan.walk_plans[0] == (2 if len(levels) >= 3 else len(levels)), plan.walk_plans
    _check_planes(rt, plan, y, uv, "crops %s" % (hw,), knobs=(0, 2, 8))
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert per_level.walk_plans[0] == len(levels)
    _check_planes(rt, per_level, y, uv, "crops %s, one plan per level" % (hw,), knobs=(0, 8))
    plan.close()
    per_level.close()


@pytest.mark.parametrize("depth", (12, 16))
def test_the_other_depths_on_every_route(rt, depth):
    """The depth is a runtime scalar: shift 4 and shift 0 through the walk, the unit + region kernels and a union plan's border."""
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    y, uv = pf.batch(2, 64, 66, depth, seed=depth)
    plan = rt.PyramidPlan(64, 66, 3, classic_levels((64, 66), 2.0, 3))
    _check_planes(rt, plan, y, uv, "classic 64 x 66, d %d" % depth, variant=("bt2020", "limited", "rgb"), depth=depth)
    plan.close()
    hw, center, scale = _crops()[1]
    y, uv = pf.batch(2, hw[0], hw[1], depth, seed=depth + 1)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, reference_levels(hw, center, scale))
    _check_planes(rt, plan, y, uv, "crops %s, d %d" % (hw, depth), knobs=(0, 8), variant=("bt601", "full", "bgr"), depth=depth)
    plan.close()


# ----------------------------------------------------------------------------- NV12 and the float32 path

@pytest.mark.parametrize("depth", pf.DEPTHS)
def test_shifted_bytes_give_the_nv12_pyramid_bit_for_bit(rt, depth):
    """(byte << 8) | junk surfaces, limited range: the pyramid at each depth equals silent_pyramid_nv12's on the byte surfaces and the
    float32 path's on the converted frames, on the walk and on the unit + region kernels."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, shift = (64, 66), 16 - depth
    y8, uv8 = nf.batch(2, hw[0], hw[1], seed=depth)
    rng = np.random.default_rng(depth)
    wide = [((b.astype(np.uint16) << 8) | (rng.integers(0, 1 << shift, b.shape) if shift else 0)).astype(np.uint16) for b in (y8, uv8)]
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    for variant in (("bt709", "limited", "bgr"), ("bt601", "limited", "rgb")):
        kw8 = dict(rgb_frame_format="nv12", nv12_matrix=variant[0], nv12_range=variant[1], nv12_order=variant[2])
        m, oy, oc = pf.coefficients(*variant, depth)
        f32 = _t(pf.convert(wide[0], wide[1], m, oy, oc, shift)).cuda(0)
        for knob in (0, 2):
            with rt.tuning(TUNE_PYRAMID, knob):
                got = plan.run(_surfaces(wide[0], wide[1], 0xFF)[1], **_kw(variant, depth))
                _same(got, plan.run(_dev(y8, uv8), **kw8), "d %d %s knob %d: against silent_pyramid_nv12 on the bytes" % (depth, variant, knob))
                _same(got, plan.run(f32), "d %d %s knob %d: against the float32 path" % (depth, variant, knob))
    plan.close()


def test_against_the_oracle_on_the_converted_frame(rt):
    """Directly, not through the float32 path: so.classic_pyramid of the restatement's frame, within the zoom's rounding bound."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (136, 240), 2.0, 4
    y, uv = pf.batch(2, hw[0], hw[1], 10, seed=n)
    m, oy, oc = pf.coefficients(*DEFAULT, 10)
    frames = pf.convert(y, uv, m, oy, oc, 6)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(_surfaces(y, uv, 0xFF)[1], **P010)
    for f in range(2):
        want = so.classic_pyramid(frames[f], scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="p010 frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


def test_chroma_offsets_past_2_31(rt):
    """Two 64 x 66 frames whose CHROMA planes lie 2^31 + 4100 bytes apart inside one uninitialised 2.2 GiB allocation (_dev form), the
    luma planes packed: frame 1's chroma address needs the 64-bit frame term on every route -- a 32-bit one would read frame 0's."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 66)
    stride, row = (1 << 30) + 2050, hw[1] + 6                  # ELEMENTS: 2^31 + 4100 and 144 bytes
    span = stride + (hw[0] // 2 - 1) * row + hw[1]
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * span + (1 << 28):
        pytest.skip("not enough free device memory for a 2.2 GiB allocation")
    big = torch.empty(span + 16, dtype=torch.int16, device="cuda:0")
    shape, strides = (2, hw[0] // 2, hw[1] // 2, 2), (stride, row, 2, 1)
    y, uv = pf.batch(2, hw[0], hw[1], 10, seed=3)
    assert not np.array_equal(uv[0], uv[1])
    torch.as_strided(big, shape, strides, 3).copy_(_t(uv.view(np.int16)).cuda(0))     # (the same bits)
    uv_view = torch.as_strided(big.view(torch.uint16), shape, strides, 3)
    dy = _t(y).cuda(0)
    assert uv_view[1].data_ptr() - uv_view[0].data_ptr() == (1 << 31) + 4100 and uv_view.data_ptr() % 4 == 2
    m, oy, oc = pf.coefficients(*DEFAULT, 10)
    f32 = _t(pf.convert(y, uv, m, oy, oc, 6)).cuda(0)
    _same(rt.p010_to_rgb((dy, uv_view), hw), f32, "uv_frame_stride 2^31 + 4100, conversion")
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same(plan.run((dy, uv_view), **P010), plan.run(f32), "uv_frame_stride 2^31 + 4100, PYRAMID knob %d" % knob)
    plan.close()
    del uv_view, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals

def test_refusals_of_the_wrapper(rt):
    """The planes pass as they are; the C entry point's own refusals arrive as ValueError with its text."""
    import torch
    from pysilent_amd import _lib
    y, uv = pf.batch(2, 40, 48)
    dy, du = _dev(y, uv)
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    swapped = torch.as_strided(du, du.shape, (du.stride(0), du.stride(1), 1, 2))
    for bad, text in (((_t(y.astype(np.float32)).cuda(0), du), "uint16"), ((_t(y.astype(np.uint8)).cuda(0), du), "uint16"), ((dy, du[:1]), "chroma plane"),
                      ((dy[:, :38], du), "luma plane"), ((dy, uv), "must either be"), (dy, "pair"), ((dy, swapped), "adjacent")):
        with pytest.raises((ValueError, TypeError), match=text):
            plan.run(bad, **P010)
    with pytest.raises(ValueError, match="rgb_frame_format='p010' does not combine with rgb_frame_dtype='uint8'"):
        plan.run((dy, du), rgb_frame_dtype="uint8", **P010)
    with pytest.raises(ValueError, match="nv12_matrix must be 'bt601', 'bt709' or a 3 x 3 array, got 'bt2020'"):
        plan.run(_dev(*nf.batch(2, 40, 48)), rgb_frame_format="nv12", nv12_matrix="bt2020")
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_format='p012' is for mode 'rgb'"):
        gray.run((dy, du), rgb_frame_format="p012")
    odd = rt.PyramidPlan(40, 47, 3, [(0, 0, 40, 47, 40, 47, 40, 47)])
    with pytest.raises(ValueError, match="rgb_frame_format='p016' needs even H and W"):
        odd.run((dy, du), rgb_frame_format="p016")
    lib, ctx = _lib.load(), plan.ctx
    out = torch.empty(2 * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
    optr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, oy, oc = pf.coefficients(*DEFAULT, 10)
    good = rt.p010_frames_of((dy, du), (40, 48), m, oy, oc, 10)[0]

    def call(handle, frames, n, pyr=optr):
        ctx.check(lib.silent_pyramid_p010_dev(ctx.handle, handle, _lib.p010_ptr(frames), n, pyr, stream))

    call(plan.handle, good, 2)
    for args, text in (((plan.handle, good[:2] + (94,) + good[3:], 2), r"silent_pyramid_p010: y_row_stride is below 2 \* W"),
                       ((plan.handle, good[:4] + (80,) + good[5:], 2), r"silent_pyramid_p010: uv_row_stride is below 2 \* W"),
                       ((plan.handle, good[:5] + (1800,) + good[6:], 2), "silent_pyramid_p010: uv_frame_stride is below"),
                       ((plan.handle, good[:6] + ([float("nan")] * 9,) + good[7:], 2), "silent_pyramid_p010: m, oy and oc must be finite"),
                       ((plan.handle, (good[0] + 1,) + good[1:], 2), "silent_pyramid_p010: y and uv must be 2-byte aligned"),
                       ((plan.handle, good[:5] + (good[5] + 1,) + good[6:], 2), "silent_pyramid_p010: a stride is odd"),
                       ((plan.handle, good[:9] + (7,), 2), "silent_pyramid_p010: shift must be 0 .. 6"),
                       ((odd.handle, good, 2), "silent_pyramid_p010: P010 frames need even H and W"),
                       ((plan.handle, good, 0), "silent_pyramid_p010: n_frames must be >= 1"),
                       ((plan.handle, good, 2, None), "silent_pyramid_p010: NULL pointer"),
                       ((gray.handle, good, 2), r"single-channel plan reads the luma plane through silent_pyramid_view16\)")):
        with pytest.raises(ValueError, match=text):
            call(*args)
    torch.cuda.synchronize()
    for p in (plan, gray, odd):
        p.close()


# ----------------------------------------------------------------------------- the pipeline

PIPES = [((136, 240), dict(n_levels=4, scale=2.0)), ((480, 640), dict(center_dimensions=(288, 192), scale=E5))]


@pytest.mark.parametrize("hw,geometry", PIPES, ids=["classic-136x240", "reference-480x640"])
def test_pipeline_p010_surfaces(rt, hw, geometry):
    """LineEndPipeline(mode="rgb", rgb_frame_format="p010", selection=True): step((y, uv)) reads the planes in place; pyramid, orient,
    line_end and keypoints equal the float32 pipeline's on p010_to_rgb(...) -- which is the restatement's frames -- bit for bit, under
    both fills; step_host gives the same; p010_planes on [n, H * 3 / 2, 1024] uint16 surfaces gives the same as explicit planes."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    from pysilent_amd.util.zoom import p010_planes
    batch = 2
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **geometry)
    y, uv = pf.batch(4, hw[0], hw[1], 10, seed=11)
    m, oy, oc = pf.coefficients(*DEFAULT, 10)
    batches = [(y[0:2], uv[0:2]), (y[2:4], uv[2:4])]
    ref = LineEndPipeline(hw, **kw)
    want = []
    for b in batches:
        converted = rt.p010_to_rgb(_dev(*b), hw, depth=10)
        _same(converted, pf.convert(b[0], b[1], m, oy, oc, 6), "p010_to_rgb")
        ref.step(converted)
        want.append(_outputs(ref))
    assert {n for n, _ in want[0]} >= {"pyramid", "orient", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(want[0], want[1]) if a.shape == b.shape)
    assert ref.rgb_frame_format == "interleaved" and "P010" not in ref.launch_summary()

    pipe = LineEndPipeline(hw, rgb_frame_format="p010", **kw)
    assert pipe.rgb_frame_format == "p010" and pipe.rgb_frame_dtype == "float32" and pipe.frame_dtype == "float32"
    assert "P010 read in place" in pipe.launch_summary() and pipe.launch_summary().startswith(ref.launch_summary())
    px = hw[0] * hw[1] if pipe.crop_px is None else pipe.crop_px
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 12 * px + 3 * px
    assert pipe.pyramid_bytes_per_frame() == ref.pyramid_bytes_per_frame() - 12 * hw[0] * hw[1] + 3 * hw[0] * hw[1]
    for fill in pf.FILLS:
        for i, b in enumerate(batches):
            pipe.step(_surfaces(b[0], b[1], fill)[1])
            _same_outputs(_outputs(pipe), want[i], "step, fill 0x%02X, batch %d" % (fill, i))
    pipe.step(_dev(*batches[1]))
    _same_outputs(_outputs(pipe), want[1], "step on contiguous planes")
    for i in (0, 1, 0):
        pipe.step_host(batches[i])
        _same_outputs(_outputs(pipe), want[i], "step_host, batch %d" % i)
    pipe.step_host(pf.views(*pf.place(batches[1][0], batches[1][1], 0xFF), batch, hw[0], hw[1]))
    _same_outputs(_outputs(pipe), want[1], "step_host on pitched host planes")
    # decoder surfaces: luma rows, chroma rows directly below, 2048-byte pitch (1024 elements); filled on the host
    host_surf = np.full((batch, hw[0] * 3 // 2, 1024), 0xA5A5, np.uint16)
    hy, hu = p010_planes(host_surf, hw[0], hw[1])
    hy[...] = batches[0][0]
    hu[...] = batches[0][1]
    surf = _t(host_surf).cuda(0)
    sy, su = p010_planes(surf, hw[0], hw[1])
    assert sy.data_ptr() == surf.data_ptr() and su.data_ptr() == surf.data_ptr() + hw[0] * 2048 and su.stride() == (surf.stride(0), 1024, 2, 1)
    pipe.step((sy, su))
    _same_outputs(_outputs(pipe), want[0], "step on p010_planes of pitched surfaces")
    for bad, text in (((_t(batches[0][0].astype(np.float32)).cuda(0), su), "uint16"), ((sy[:1], su[:1]), "pair"), (sy, "pair")):
        with pytest.raises(ValueError, match=text):
            pipe.step(bad)
    with pytest.raises(ValueError, match="pair of uint16 arrays"):
        pipe.step_host(batches[0][0])
    with pytest.raises(ValueError, match="pair of uint16 arrays"):
        pipe.step_host(tuple(p.astype(np.uint8) for p in batches[0]))
    with pytest.raises((ValueError, AttributeError, TypeError)):
        ref.step((sy, su))
    for p in (ref, pipe):
        p.close()


@pytest.mark.parametrize("depth,variant", [(10, ("bt2020", "limited", "rgb")), (12, ("bt2020", "full", "bgr")), (16, ("bt601", "full", "rgb")),
                                           (10, "array")], ids=["p010-bt2020", "p012-bt2020-full", "p016-bt601-full", "p010-array"])
def test_pipeline_other_coefficients(rt, depth, variant):
    """nv12_matrix / nv12_range / nv12_order and the depth of the format's name reach the kernels: against the float32 pipeline on that
    conversion."""
    from pysilent_amd.pipeline import LineEndPipeline
    hw = (136, 240)
    kw = dict(mode="rgb", batch=2, device=0, selection=True, placement=None, n_levels=4, scale=2.0)
    y, uv = pf.batch(2, hw[0], hw[1], depth, seed=5)
    s = np.float32(2.0 ** (depth - 8))
    if variant == "array":
        a = np.array([[1.1, 1.9, 0.1], [1.2, -.4, -.7], [.9, 0.0, 1.6]], np.float32)
        keywords = dict(rgb_frame_format=FORMAT[depth], nv12_matrix=a, nv12_range="limited")
        m, oy, oc = a / s, 16 * s, 128 * s
    else:
        keywords = _kw(variant, depth)
        m, oy, oc = pf.coefficients(*variant, depth)
    ref, pipe = LineEndPipeline(hw, **kw), LineEndPipeline(hw, **dict(kw, **keywords))
    ref.step(_t(pf.convert(y, uv, m, oy, oc, 16 - depth)).cuda(0))
    pipe.step(_surfaces(y, uv, 0x00)[1])
    _same_outputs(_outputs(pipe), _outputs(ref), "%s d %d" % (variant, depth))
    for p in (ref, pipe):
        p.close()
