"""Strided uint8 colour views for 3-channel plans on the GPU (silent_pyramid_rgb8_view[_dev], PyramidPlan.run(rgb_frame_dtype="uint8",
rgb_frame_layout="strided"), LineEndPipeline(mode="rgb", rgb_frame_dtype="uint8", rgb_frame_layout="strided")): the pyramid is that
of the packed uint8 call on view.contiguous() BIT FOR BIT -- host form and _dev form, on every route of launch_pyramid3 (the walk
kernel at 36 / 32 / 28 / 24 pixels per wave and 4 / 7 general levels, union and per-level plans, the border pixels inside and behind
the walk's launch, the unit + region kernels) -- and with it every map and keypoint of the RGB pipeline.  The frames are those of
tests/rgb_uint8_frames.py in the views of tests/rgb_strided_views.py, each placed into a parent filled with 0x00 and then with 0xFF
(tests/test_rgb_strided_host.py shows what they can see)."""
import ctypes as C
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_strided_views as rv
import rgb_uint8_frames as rf
import silent_oracle as so
from conftest import assert_close
from test_rgb_uint8 import _outputs, _same, _same_outputs, _t

pytestmark = pytest.mark.gpu
RGB8 = dict(rgb_frame_dtype="uint8")
STRIDED = dict(rgb_frame_dtype="uint8", rgb_frame_layout="strided")
E5 = math.e ** .5
TWO = ("bgra", "odd-pitch bgr")             # run on every geometry; all of rv.KINDS on (135, 240) and (270, 482)


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _device_view(kind, frames, fill):
    """(host parent, host view, device view) of ``frames`` in a parent filled with ``fill``."""
    B, H, W, _ = frames.shape
    parent = rv.place(kind, frames, fill)
    dev = rv.as_torch(_t(parent).cuda(0), kind, B, H, W)
    if kind.startswith("bgra"):
        assert dev.data_ptr() % 4 == (1 if kind.endswith("byte 1") else 0) and dev.stride() == (H * W * 4, W * 4, 4, 1)
    assert dev.is_contiguous() == (kind == "packed")
    return parent, rv.as_numpy(parent, kind, B, H, W), dev


def _check_views(rt, plan, frames, kinds, what, knobs=(0, 2)):
    """_dev form and host form on each kind of view, under both fills and each PYRAMID knob, against the packed uint8 call on the
    compacted frames (view.contiguous() is `frames`: asserted)."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    packed = _t(frames).cuda(0)
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(packed, **RGB8)
            for kind in kinds:
                got = []
                for fill in rv.FILLS:
                    _, host, dev = _device_view(kind, frames, fill)
                    assert torch.equal(dev.contiguous(), packed)
                    tag = "%s, %s, fill 0x%02X, PYRAMID knob %d" % (what, kind, fill, knob)
                    got_dev, got_host = plan.run(dev, **STRIDED), plan.run(host, **STRIDED)
                    assert got_dev.on_device and not got_host.on_device and got_dev.channels == got_host.channels == 3
                    _same(got_dev, want, tag + ", _dev form")
                    _same(got_host, want, tag + ", host form")
                    got.append(got_dev)
                _same(got[0], got[1], "%s, %s, PYRAMID knob %d: the two fills" % (what, kind, knob))


# ----------------------------------------------------------------------------- classic pyramids

CLASSIC = [((135, 240), 2.0, 4, (1, 36)),             # PX 36, G 4, a ragged second strip (240 = 144 + 96)
           ((270, 480), 2.0, 8, (1, 36)),             # G 7
           ((40, 8), 2.0, 2, (1, 36)),                # narrower than a wave tile
           ((135, 241), 2.0, 4, (1, 36)),             # 3 W mod 4 = 3
           ((64, 66), 2.0, 3, (1, 36)),               # 3 W mod 4 = 2
           ((97, 999), 2.0, 4, (1, 36)),              # 3 W mod 4 = 1, 7 strips
           ((135, 240), 1.7, 4, (1, 32)),             # PX 32
           ((270, 480), 2 ** .5, 6, (1, 28)),         # PX 28
           ((200, 300), 2 ** (1 / 3), 5, (1, 24)),    # PX 24
           ((270, 480), 2 ** .5, 10, (0, 0))]         # 9 general levels: the unit + region kernels


@pytest.mark.parametrize("hw,scale,n,route", CLASSIC, ids=["%dx%d-s%.3g-n%d" % (c[0] + c[1:3]) for c in CLASSIC])
def test_classic_pyramids_bit_identical_to_the_packed_uint8_call(rt, hw, scale, n, route):
    from pysilent_amd.util.zoom.from_image import classic_levels
    frames = rf.batch(2, hw[0], hw[1], seed=n)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    assert plan.walk_plans == route
    kinds = rv.KINDS if (hw, scale) == ((135, 240), 2.0) else TWO
    _check_views(rt, plan, frames, kinds, "classic %s scale %.3g n %d" % (hw, scale, n))
    plan.close()


# ----------------------------------------------------------------------------- crop layouts

CROPS = [((480, 640), (288, 192), E5),                # the reference's defaults on its camera frame
         ((270, 480), (61, 45), 2.0),                 # odd extents and crop offsets: alignment shift 1 .. 3
         ((270, 482), (61, 45), 2.0)]                 # W % 4 != 0


@pytest.mark.parametrize("hw,center,scale", CROPS, ids=["%dx%d" % c[0] for c in CROPS])
def test_crop_layouts_bit_identical_to_the_packed_uint8_call(rt, hw, center, scale):
    """The union plan with its border pixels inside the walk's launch (knob 0) and behind it (knob 8), the unit + region kernels
    (knob 2), and one plan per level (knob 4 at plan creation)."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import reference_levels
    levels = reference_levels(hw, center, scale)
    frames = rf.batch(2, hw[0], hw[1], seed=len(levels))
    kinds = rv.KINDS if hw == (270, 482) else TWO
    plan = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    n_plans, px = plan.walk_plans
    assert n_plans == (2 if len(levels) >= 3 else len(levels)) and px in (32, 36), (n_plans, px)
    _check_views(rt, plan, frames, kinds, "crops %s" % (hw,), knobs=(0, 2, 8))
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert per_level.walk_plans[0] == len(levels)
    _check_views(rt, per_level, frames, kinds, "crops %s, one plan per level" % (hw,), knobs=(0, 8))
    _same(per_level.run(_device_view("bgra", frames, 0xFF)[2], **STRIDED), plan.run(frames, **RGB8),
          "crops %s: per-level plans on a view against the union plan" % (hw,))
    plan.close()
    per_level.close()


# ----------------------------------------------------------------------------- against the oracle

def test_against_the_oracle_on_the_widened_compacted_frame(rt):
    """Directly, not through the packed path: so.classic_pyramid of the widened frame, within the zoom's rounding bound (the statement
    of test_rgb_uint8.test_against_the_oracle_on_the_widened_frame, on a BGRA view in a parent of 0xFF)."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (135, 240), 2.0, 4
    frames = rf.batch(2, hw[0], hw[1], seed=n)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(_device_view("bgra", frames, 0xFF)[2], **STRIDED)
    for f in range(2):
        want = so.classic_pyramid(frames[f].astype(np.float32), scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="rgb8 view frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


# ----------------------------------------------------------------------------- 64-bit frame term

def test_frame_stride_past_2_31(rt):
    """Two 64 x 66 frames 2^31 + 4099 bytes apart inside one uninitialised 2.2 GiB allocation (_dev form), rows of 3 W + 5 bytes: frame
    1's address needs the 64-bit frame term on every route (the walk kernel, the unit + region kernels), and 4099 makes it odd."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 66)
    stride, row = (1 << 31) + 4099, 3 * hw[1] + 5
    span = stride + (hw[0] - 1) * row + (hw[1] - 1) * 3 + 3
    big = torch.empty(span + 16, dtype=torch.uint8, device="cuda:0")
    view = torch.as_strided(big, (2, hw[0], hw[1], 3), (stride, row, 3, 1), 5)
    frames = rf.batch(2, hw[0], hw[1], seed=3)
    px = _t(frames).cuda(0)
    view.copy_(px)
    assert view.data_ptr() == big.data_ptr() + 5 and view[1].data_ptr() - view[0].data_ptr() == stride
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same(plan.run(view, **STRIDED), plan.run(px, **RGB8), "frame_stride 2^31 + 4099, PYRAMID knob %d" % knob)
    plan.close()
    del view, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals

def test_refusals_of_the_wrapper(rt):
    """A view passes as it is: anything that is not a uint8 [n, H, W, 3] view with positive strides and channel stride 1 is a
    ValueError, never converted; a single-channel plan refuses the keyword; and the C entry point's own refusals arrive as ValueError
    with its text."""
    import torch
    from pysilent_amd import _lib
    frames = rf.batch(2, 40, 48)
    dev = _t(frames).cuda(0)
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    planar = torch.zeros((2, 3, 40, 48), dtype=torch.uint8, device="cuda:0").permute(0, 2, 3, 1)
    for bad, text in ((planar, "adjacent bytes"), (frames[..., ::-1], "adjacent bytes"), (dev[:1].expand(2, 40, 48, 3), "positive"),
                      (torch.as_strided(dev, (2, 40, 48, 3), (5760, 144, 2, 1)), "overlap"),
                      (dev.to(torch.float32), "uint8"), (frames.astype(np.int8), "uint8"), (frames.astype(np.float32), "uint8"),
                      (np.broadcast_to(frames[:1], frames.shape), "positive")):
        with pytest.raises(ValueError, match=text):
            plan.run(bad, **STRIDED)
    for bad in (dev[:, :, ::2], dev[..., :2], frames[:, :39], dev[0]):
        with pytest.raises(ValueError, match=r"\[n, 40, 48, 3\]"):
            plan.run(bad, **STRIDED)
    with pytest.raises(ValueError, match="rgb_frame_layout='strided' needs rgb_frame_dtype='uint8'"):
        plan.run(dev, rgb_frame_layout="strided")
    with pytest.raises(ValueError, match=r"rgb_frame_dtype='uint8' does not combine with frame_layout='strided' \(packed frames only\)"):
        plan.run(dev, frame_layout="strided", **STRIDED)
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_dtype"):
        gray.run(dev, **STRIDED)
    with pytest.raises(ValueError, match="rgb_frame_layout='strided' is for mode 'rgb'"):
        gray.run(dev[..., 0], frame_dtype="uint8", rgb_frame_layout="strided")
    # the C refusals, as the wrapper maps them
    lib, ctx = _lib.load(), plan.ctx
    out = torch.empty(2 * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
    optr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = rt.frame_view_of(dev, 3, "uint8")

    def call(handle, view, n, pyr=optr):
        ctx.check(lib.silent_pyramid_rgb8_view_dev(ctx.handle, handle, _lib.view_ptr(view), n, pyr, stream))

    call(plan.handle, good, 2)
    for args, text in (((plan.handle, (good[0], 1) + good[2:], 2), "silent_pyramid_rgb8_view: view channels must be 3"),
                       ((plan.handle, good[:2] + (2,) + good[3:], 2), "silent_pyramid_rgb8_view: view pixel_stride is below channels"),
                       ((plan.handle, good[:3] + (140,) + good[4:], 2), "silent_pyramid_rgb8_view: view row_stride is below"),
                       ((plan.handle, good[:4] + (5000,), 2), "silent_pyramid_rgb8_view: view frame_stride is below"),
                       ((plan.handle, good, 0), "silent_pyramid_rgb8_view: n_frames must be >= 1"),
                       ((plan.handle, good, 2, None), "silent_pyramid_rgb8_view: NULL pointer"),
                       ((gray.handle, good, 2), r"single-channel plan takes them through silent_pyramid_view\)")):
        with pytest.raises(ValueError, match=text):
            call(*args)
    torch.cuda.synchronize()
    plan.close()
    gray.close()


# ----------------------------------------------------------------------------- the pipeline

PIPES = [((135, 240), dict(n_levels=4, scale=2.0)), ((480, 640), dict(center_dimensions=(288, 192), scale=E5))]


@pytest.mark.parametrize("hw,geometry", PIPES, ids=["classic-135x240", "reference-480x640"])
def test_pipeline_strided_colour_views(rt, hw, geometry):
    """LineEndPipeline(mode="rgb", rgb_frame_dtype="uint8", rgb_frame_layout="strided", selection=True): step(view) reads a BGRA view
    and a region of larger frames in place; pyramid, orient, line_end and keypoints equal the packed uint8 pipeline's on the compacted
    frames bit for bit, under both fills; a contiguous tensor is a view too; step_host is unchanged."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    batch = 2
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **geometry)
    all_frames = rf.batch(4, hw[0], hw[1], seed=11)
    batches = [np.array(all_frames[0:2]), np.array(all_frames[2:4])]
    ref = LineEndPipeline(hw, rgb_frame_dtype="uint8", **kw)
    want = []
    for b in batches:
        ref.step(_t(b).cuda(0))
        want.append(_outputs(ref))
    assert {n for n, _ in want[0]} >= {"pyramid", "orient", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(want[0], want[1]) if a.shape == b.shape)
    assert ref.rgb_frame_layout == "packed" and "strided" not in ref.launch_summary()

    pipe = LineEndPipeline(hw, rgb_frame_layout="strided", **dict(kw, rgb_frame_dtype="uint8"))
    assert pipe.rgb_frame_layout == "strided" and pipe.rgb_frame_dtype == "uint8" and pipe.frame_dtype == "uint8" and pipe.frame_layout == "packed"
    assert "read in place from a strided view" in pipe.launch_summary() and pipe.launch_summary().startswith(ref.launch_summary())
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame()
    assert pipe.pyramid_bytes_per_frame() == ref.pyramid_bytes_per_frame()
    for kind in ("bgra", "region at (7, 5)"):
        for fill in rv.FILLS:
            for i, b in enumerate(batches):
                view = _device_view(kind, b, fill)[2]
                assert not view.is_contiguous()
                pipe.step(view)
                _same_outputs(_outputs(pipe), want[i], "step, %s, fill 0x%02X, batch %d" % (kind, fill, i))
    pipe.step(_t(batches[1]).cuda(0))
    _same_outputs(_outputs(pipe), want[1], "step on a contiguous tensor (a packed view)")
    pipe.step_host(batches[0])
    _same_outputs(_outputs(pipe), want[0], "step_host (its staging copy packs)")
    with pytest.raises(ValueError, match="uint8"):
        pipe.step(_t(batches[0]).cuda(0).to(torch.float32))
    with pytest.raises(ValueError, match="adjacent bytes"):
        pipe.step(torch.zeros((batch, 3) + hw, dtype=torch.uint8, device="cuda:0").permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match="contiguous"):
        ref.step(_device_view("bgra", batches[0], 0)[2])
    for p in (ref, pipe):
        p.close()
