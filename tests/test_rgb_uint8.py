"""Packed uint8 colour frames for 3-channel plans on the GPU (silent_pyramid_rgb8[_dev], PyramidPlan.run(rgb_frame_dtype="uint8"),
LineEndPipeline(mode="rgb", rgb_frame_dtype="uint8")): the pyramid is that of the float32-frame call on frames.astype(float32) BIT FOR
BIT -- host form and _dev form, under SILENT_TUNE_PYRAMID 0 and 2, on every route of launch_pyramid (the walk kernel at 36 / 32 / 28 /
24 pixels per wave and 4 / 7 general levels, its dword and one-byte loaders, union and per-level plans, the border pixels inside and
behind the walk's launch, the unit + region kernels) -- and with it every map and keypoint of the RGB pipeline.  The frames are
those of tests/rgb_uint8_frames.py (tests/test_rgb_uint8_host.py shows what they can see)."""
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_uint8_frames as rf
import silent_oracle as so
from conftest import assert_close

pytestmark = pytest.mark.gpu
RGB8 = dict(rgb_frame_dtype="uint8")
E5 = math.e ** .5


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(x):
    """The float32 ndarray behind a PackedPyramid, tensor or ndarray."""
    x = x.data if type(x).__name__ == "PackedPyramid" else x
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x)


def _bits(x):
    return _np(x).view(np.uint32)


def _same(got, want, what):
    """np.array_equal (the frames are bytes: no NaN anywhere), and the same bit patterns (-0.0 against 0.0 would pass the first)."""
    g, w = _np(got), _np(want)
    assert g.shape == w.shape and g.dtype == w.dtype == np.float32, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.view(np.uint32).reshape(-1) != w.view(np.uint32).reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d" % (what, bad.size, g.size, int(bad[0]))
    assert np.array_equal(g, w), what


def _check_plan(rt, plan, frames, what, knobs=(0, 2)):
    """uint8 host form and _dev form against the float32-frame call on the widened frames, under each PYRAMID knob."""
    from pysilent_amd._lib import TUNE_PYRAMID
    f32 = _t(frames.astype(np.float32)).cuda(0)
    dev = _t(frames).cuda(0)
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            got_dev = plan.run(dev, **RGB8)
            got_host = plan.run(frames, **RGB8)
        assert got_dev.on_device and not got_host.on_device and got_dev.channels == got_host.channels == 3
        _same(got_dev, want, "%s, _dev form, PYRAMID knob %d" % (what, knob))
        _same(got_host, want, "%s, host form, PYRAMID knob %d" % (what, knob))


# ----------------------------------------------------------------------------- classic pyramids

CLASSIC = [((135, 240), 2.0, 4, (1, 36)),             # PX 36, G 4, a ragged second strip (240 = 144 + 96)
           ((270, 480), 2.0, 8, (1, 36)),             # G 7
           ((40, 8), 2.0, 2, (1, 36)),                # narrower than a wave tile
           ((135, 241), 2.0, 4, (1, 36)),             # 3 W mod 4 = 3: the one-byte loader
           ((64, 66), 2.0, 3, (1, 36)),               # 3 W mod 4 = 2
           ((97, 999), 2.0, 4, (1, 36)),              # 3 W mod 4 = 1, 7 strips
           ((135, 240), 1.7, 4, (1, 32)),             # PX 32
           ((270, 480), 2 ** .5, 6, (1, 28)),         # PX 28
           ((200, 300), 2 ** (1 / 3), 5, (1, 24)),    # PX 24
           ((270, 480), 2 ** .5, 10, (0, 0))]         # 9 general levels: the unit + region kernels


@pytest.mark.parametrize("hw,scale,n,route", CLASSIC, ids=["%dx%d-s%.3g-n%d" % (c[0] + c[1:3]) for c in CLASSIC])
def test_classic_pyramids_bit_identical_to_the_float32_frame_call(rt, hw, scale, n, route):
    from pysilent_amd.util.zoom.from_image import classic_levels
    frames = rf.batch(2, hw[0], hw[1], seed=n)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    assert plan.walk_plans == route
    _check_plan(rt, plan, frames, "classic %s scale %.3g n %d" % (hw, scale, n))
    plan.close()


# ----------------------------------------------------------------------------- crop layouts

CROPS = [((480, 640), (288, 192), E5),                # the reference's defaults on its camera frame
         ((270, 480), (61, 45), 2.0),                 # odd extents and crop offsets: alignment shift 1 .. 3
         ((270, 482), (61, 45), 2.0),                 # W % 4 != 0: the one-byte loader on crops
         ((97, 132), (32, 24), 1.7)]


@pytest.mark.parametrize("hw,center,scale", CROPS, ids=["%dx%d" % c[0] for c in CROPS])
def test_crop_layouts_bit_identical_to_the_float32_frame_call(rt, hw, center, scale):
    """The union plan with its border pixels inside the walk's launch (knob 0) and behind it (knob 8), the unit + region kernels
    (knob 2), and one plan per level (knob 4 at plan creation)."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import reference_levels
    levels = reference_levels(hw, center, scale)
    frames = rf.batch(2, hw[0], hw[1], seed=len(levels))
    plan = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    n_plans, px = plan.walk_plans
    assert n_plans == (2 if len(levels) >= 3 else len(levels)) and px in (32, 36), (n_plans, px)
    _check_plan(rt, plan, frames, "crops %s" % (hw,), knobs=(0, 2, 8))
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert per_level.walk_plans[0] == len(levels)
    _check_plan(rt, per_level, frames, "crops %s, one plan per level" % (hw,), knobs=(0, 8))
    _same(per_level.run(frames, **RGB8), plan.run(frames.astype(np.float32)), "crops %s: per-level plans against the union plan" % (hw,))
    plan.close()
    per_level.close()


# ----------------------------------------------------------------------------- pointer alignment

@pytest.mark.parametrize("hw", [(135, 240), (64, 66)], ids=lambda hw: "%dx%d" % hw)
def test_misaligned_frames_pointer(rt, hw):
    """`frames` has no alignment requirement: the batch at byte offsets 1, 2 and 3 of a larger device allocation gives the pyramid of
    offset 0 (W % 4 == 0: the dword loader is legal at offset 0 only; the region kernel's group loads likewise)."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    frames = rf.batch(2, hw[0], hw[1], seed=5)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    f32 = _t(frames.astype(np.float32)).cuda(0)
    big = torch.full((frames.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big.data_ptr() % 4 == 0
    flat = _t(frames.reshape(-1)).cuda(0)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            for off in (0, 1, 2, 3):
                big.fill_(0xA5)
                view = big[off:off + frames.size]
                view.copy_(flat)
                dev = view.view(frames.shape)
                assert dev.is_contiguous() and dev.data_ptr() % 4 == off
                _same(plan.run(dev, **RGB8), want, "%s at byte offset %d, PYRAMID knob %d" % (hw, off, knob))
    plan.close()


# ----------------------------------------------------------------------------- against the oracle

def test_against_the_oracle_on_the_widened_frame(rt):
    """Directly, not through the float32 path: so.classic_pyramid of the widened frame, within the zoom's rounding bound."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (135, 240), 2.0, 4
    frames = rf.batch(2, hw[0], hw[1], seed=n)
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(_t(frames).cuda(0), **RGB8)
    for f in range(2):
        want = so.classic_pyramid(frames[f].astype(np.float32), scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="rgb8 frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


def test_refusals_of_the_wrapper(rt):
    """Frames pass as they are: anything that is not uint8 [n, H, W, 3] is refused, never converted; a single-channel plan refuses
    the keyword."""
    frames = rf.batch(2, 40, 48)
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    for bad in (frames.astype(np.float32), frames.astype(np.int8), _t(frames.astype(np.float32)).cuda(0), _t(frames).cuda(0)[:, :, ::2]):
        with pytest.raises(ValueError):
            plan.run(bad, **RGB8)
    with pytest.raises(ValueError, match=r"\[n, 40, 48, 3\]"):
        plan.run(frames[:, :, :, :1], **RGB8)
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_dtype"):
        gray.run(frames, **RGB8)
    plan.close()
    gray.close()


# ----------------------------------------------------------------------------- the pipeline

class _Counting(object):
    """The loaded library with a count of the calls of one entry point."""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def call(*args):
            self.calls += 1
            return fn(*args)
        return call


def _outputs(pipe):
    """(name, bits) of everything the pipeline returns: pyramid, orient, line_end, keypoints, keypoint_counts."""
    out = pipe.outputs()
    named = []
    for k in sorted(out):
        v = out[k]
        if k == "keypoints":
            named += [("keypoints of frame %d" % f, np.ascontiguousarray(a)) for f, a in enumerate(v)]
        elif k == "keypoint_counts":
            named.append((k, np.ascontiguousarray(v)))
        else:
            named.append((k, _bits(v)))
    return named


def _same_outputs(got, want, what):
    assert [n for n, _ in got] == [n for n, _ in want], what
    for (n, g), (_, w) in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs" % (what, n)


PIPES = [((135, 240), dict(n_levels=4, scale=2.0)), ((480, 640), dict(center_dimensions=(288, 192), scale=E5))]


@pytest.mark.parametrize("hw,geometry", PIPES, ids=["classic-135x240", "reference-480x640"])
def test_pipeline_uint8_colour_frames(rt, monkeypatch, hw, geometry):
    """LineEndPipeline(mode="rgb", rgb_frame_dtype="uint8", selection=True): pyramid, orient, line_end and keypoints equal the float32
    pipeline's on the widened frames bit for bit -- in step, step_host (pinned and pageable source), overlap="force" and after the
    placement tuner; step_host never calls silent_cast_interleave_dev, its slots have no float32 buffer, and the ring holds
    2 * batch * H * W * 3 bytes of device memory."""
    import torch
    from pysilent_amd import _lib
    from pysilent_amd.pipeline import LineEndPipeline
    batch = 2
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **geometry)
    all_frames = rf.batch(4, hw[0], hw[1], seed=11)
    batches = [np.array(all_frames[0:2]), np.array(all_frames[2:4]), np.array(all_frames[[3, 0]])]
    counting = _Counting(_lib.load(), "silent_cast_interleave_dev")
    monkeypatch.setattr(_lib, "_lib", counting)

    ref = LineEndPipeline(hw, **kw)
    want = []
    for b in batches:
        ref.step(_t(b.astype(np.float32)).cuda(0))
        want.append(_outputs(ref))
    assert {n for n, _ in want[0]} >= {"pyramid", "orient", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(want[0], want[1]) if a.shape == b.shape)
    # the proxy sees the cast of the float32 pipeline's uint8 ingest
    ref.step_host(batches[0])
    _same_outputs(_outputs(ref), want[0], "float32 pipeline, step_host of uint8 frames")
    assert counting.calls == 1
    assert ref.frame_dtype == "float32" and ref.rgb_frame_dtype == "float32" and "uint8" not in ref.launch_summary()

    dev = [_t(b).cuda(0) for b in batches]
    pipe = LineEndPipeline(hw, rgb_frame_dtype="uint8", **kw)
    assert pipe.frame_dtype == "uint8" and pipe.rgb_frame_dtype == "uint8" and "uint8 frames read in place" in pipe.launch_summary()
    assert pipe.frame_shape == (hw[0], hw[1], 3) and pipe.channels == 3
    assert pipe._synthetic_frames().dtype == torch.uint8 and pipe._synthetic_frames().shape == (batch, hw[0], hw[1], 3)
    n_el = (pipe.crop_px if pipe.crop_px is not None else hw[0] * hw[1]) * 3
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 3 * n_el
    assert pipe.pyramid_bytes_per_frame() == ref.pyramid_bytes_per_frame() - 3 * hw[0] * hw[1] * 3
    for i in range(len(batches)):
        pipe.step(dev[i])
        _same_outputs(_outputs(pipe), want[i], "step, batch %d" % i)
    with pytest.raises(ValueError, match="uint8"):
        pipe.step(dev[0].to(torch.float32))
    with pytest.raises(ValueError, match="float32"):
        ref.step(dev[0])
    with pytest.raises(ValueError, match="uint8"):
        pipe.step_host(batches[0].astype(np.float32))

    counting.calls = 0
    for source in ("pageable", "pinned"):
        host = LineEndPipeline(hw, rgb_frame_dtype="uint8", **kw)
        srcs = [np.array(b) if source == "pageable" else _t(b).pin_memory() for b in batches]
        for i in range(len(batches)):
            host.step_host(srcs[i])
            _same_outputs(_outputs(host), want[i], "step_host (%s), batch %d" % (source, i))
        for i in (1, 2, 0, 2, 1):                       # back to back through the ring of two slots, no synchronisation in between
            host.step_host(srcs[i])
        _same_outputs(_outputs(host), want[1], "step_host (%s), back to back" % source)
        slots = host._ingest[torch.uint8]["slots"]
        assert list(host._ingest) == [torch.uint8] and len(slots) == 2
        assert all(s["f32"] is None and s["raw"].dtype == torch.uint8 for s in slots)
        assert all((s["pinned"] is None) == (source == "pinned") for s in slots)
        held = sum(t.numel() * t.element_size() for s in slots for t in (s["raw"], s["f32"]) if t is not None)
        assert held == 2 * batch * hw[0] * hw[1] * 3
        host.close()

    ov = LineEndPipeline(hw, rgb_frame_dtype="uint8", overlap="force", **kw)
    for i in range(len(batches)):
        ov.step(dev[i])
        _same_outputs(_outputs(ov), want[i], "overlap='force', batch %d" % i)
    for i in (1, 2, 0, 2, 1, 0):
        ov.step_host(batches[i])
    _same_outputs(_outputs(ov), want[0], "overlap='force' + step_host, back to back")
    assert all(s["f32"] is None for s in ov._ingest[torch.uint8]["slots"])
    ov.close()
    assert counting.calls == 0, "step_host of a uint8 pipeline launched the widening cast"

    tuned = LineEndPipeline(hw, rgb_frame_dtype="uint8", **kw)
    assert tuned.tune_placement(tries=2, steps=2, budget_s=0.3)["stopped_by"] in ("tries", "budget_s", "memory cap", "allocation failed")
    tuned.step(dev[2])
    _same_outputs(_outputs(tuned), want[2], "after the placement tuner on its own uint8 frames")
    for p in (ref, pipe, tuned):
        p.close()
