"""Raw 8-bit Bayer mosaics for 3-channel plans on the GPU (silent_bayer_to_rgb[_dev], silent_pyramid_bayer[_dev],
PyramidPlan.run(rgb_frame_format="bayer_*"), LineEndPipeline(mode="rgb", rgb_frame_format="bayer_*")): the conversion equals the NumPy
restatement of tests/rgb_bayer_frames.py BIT FOR BIT on every pattern, order and layout, and the pyramid is that of silent_pyramid on the
restatement's float32 frames bit for bit -- host form and _dev form, on every route of launch_pyramid3 (the walk kernel with its
three-row loader, union and per-level plans, the border pixels inside and behind the walk's launch, the unit + region kernels) -- and
with it every map and keypoint of the RGB pipeline.  There is no tolerance anywhere: the conversion is exact in float32.  The mosaics
lie in parents filled with 0x00 and then with 0xFF."""
import ctypes as C
import math

import numpy as np
import pytest

import err_bound as eb
import rgb_bayer_frames as bf
import silent_oracle as so
from conftest import assert_close
from test_rgb_nv12_host import odd_origin_crops
from test_rgb_uint8 import _same, _t

pytestmark = pytest.mark.gpu
E5 = math.e ** .5


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    assert bf.checks()                       # the restatement passes its three checks before anything is compared with it
    return _runtime


def _placed(s, m, fill):
    """(the parent, the host view, the device view) of the mosaic in a parent filled with ``fill``."""
    parent = bf.place(s, m, fill)
    return parent, bf.view(s, parent), bf.torch_view(s, _t(parent).cuda(0))


# ----------------------------------------------------------------------------- the conversion

class _Struct(object):
    """silent_bayer_to_rgb[_dev] called with the struct built by hand."""

    def __init__(self, rt):
        import torch
        from pysilent_amd import _lib
        self.rt, self.torch, self._lib, self.lib, self.ctx = rt, torch, _lib, _lib.load(), rt.get_context(0)

    def to_rgb(self, s, parent, pattern, order, dev):
        torch = self.torch
        n, H, W = s["n"], s["H"], s["W"]
        if dev:
            keep = _t(parent).cuda(0)
            out = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda:0")
            ptr = self._lib.bayer_ptr(bf.struct_args(s, keep.data_ptr(), pattern, order))
            self.ctx.check(self.lib.silent_bayer_to_rgb_dev(self.ctx.handle, ptr, n, H, W, C.c_void_p(out.data_ptr()),
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            return out
        out = np.empty((n, H, W, 3), np.float32)
        ptr = self._lib.bayer_ptr(bf.struct_args(s, parent.ctypes.data, pattern, order))
        self.ctx.check(self.lib.silent_bayer_to_rgb(self.ctx.handle, ptr, n, H, W, out.ctypes.data_as(C.c_void_p)))
        return out


SIZES = [(24, 34), (25, 33), (2, 2), (3, 2)]


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("layout", list(bf.LAYOUTS))
def test_conversion_equals_the_restatement_bit_for_bit(rt, layout, hw):
    """silent_bayer_to_rgb_dev and the host form, through the struct and through _runtime.bayer_to_rgb, for 4 patterns x 2 orders under
    both fills: 2 x 24 x 34; 2 x 25 x 33 (the last row and column reflect onto the other parity); 2 x 2 x 2 and 2 x 3 x 2 (every
    neighbour reflected)."""
    H, W = hw
    s = bf.spec(layout, 2, H, W)
    m = bf.batch(s, seed=1)
    c = _Struct(rt)
    for fill in bf.FILLS:
        parent, host, dev = _placed(s, m, fill)
        for pattern in bf.PATTERNS:
            for order in bf.ORDERS:
                want = bf.truth(m, pattern, order)
                tag = "%s %dx%d %s %s, fill 0x%02X" % (layout, H, W, pattern, order, fill)
                for form in (True, False):
                    _same(c.to_rgb(s, parent, pattern, order, form), want, tag + ", struct, %s form" % ("_dev" if form else "host"))
                got = rt.bayer_to_rgb(dev, (H, W), "bayer_" + pattern, order)
                assert got.is_cuda and tuple(got.shape) == (2, H, W, 3)
                _same(got, want, tag + ", _dev form")
                _same(rt.bayer_to_rgb(host, (H, W), "bayer_" + pattern, order), want, tag + ", host form")
    # [n, H, W, 1] is the same view
    _same(rt.bayer_to_rgb(dev[..., None], (H, W), "bayer_grbg"), bf.truth(m, "grbg"), "a trailing axis of one")


def test_conversion_of_a_window_is_the_conversion_of_its_bytes(rt):
    """A window at an odd row and an odd column of larger sensor images, named by bayer_window: the restatement of the window's bytes."""
    from pysilent_amd.util.zoom import bayer_window
    import torch
    rng = np.random.default_rng(5)
    sensor = rng.integers(0, 256, (2, 33, 46)).astype(np.uint8)
    dev = _t(sensor).cuda(0)
    for y0, x0 in ((3, 5), (0, 1), (1, 0)):
        fmt = bayer_window("bayer_rggb", y0, x0)
        win = dev[:, y0:y0 + 25, x0:x0 + 33]
        want = bf.truth(np.ascontiguousarray(sensor[:, y0:y0 + 25, x0:x0 + 33]), fmt[6:])
        _same(rt.bayer_to_rgb(win, (25, 33), fmt), want, "window at (%d, %d) as %s" % (y0, x0, fmt))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- pyramids

def _check_mosaics(rt, plan, pattern, n, hw, what, knobs=(0, 2), layout="pitched", order="bgr", seed=0):
    """_dev form and host form under both fills and each PYRAMID knob against silent_pyramid on the restatement's float32 frames."""
    from pysilent_amd._lib import TUNE_PYRAMID
    s = bf.spec(layout, n, hw[0], hw[1])
    m = bf.batch(s, seed=seed)
    f32 = _t(bf.truth(m, pattern, order)).cuda(0)
    kw = dict(rgb_frame_format="bayer_" + pattern, nv12_order=order)
    for knob in knobs:
        with rt.tuning(TUNE_PYRAMID, knob):
            want = plan.run(f32)
            got = []
            for fill in bf.FILLS:
                _, host, dev = _placed(s, m, fill)
                tag = "%s %s %s, fill 0x%02X, PYRAMID knob %d" % (pattern, layout, what, fill, knob)
                got_dev, got_host = plan.run(dev, **kw), plan.run(host, **kw)
                assert got_dev.on_device and not got_host.on_device and got_dev.channels == got_host.channels == 3
                _same(got_dev, want, tag + ", _dev form")
                _same(got_host, want, tag + ", host form")
                got.append(got_dev)
            _same(got[0], got[1], "%s %s, PYRAMID knob %d: the two fills" % (pattern, what, knob))


CLASSIC = [((40, 8), 2.0, 2), ((64, 66), 2.0, 3), ((136, 240), 2.0, 4), ((134, 242), 2.0, 4),
           ((40, 8), E5, 2), ((64, 66), E5, 3), ((136, 240), E5, 4), ((134, 242), E5, 4)]
# the whole list for rggb; (64, 66) and (134, 242) for the other three patterns; odd extents (65, 67)
CLASSIC_CASES = [("rggb", c) for c in CLASSIC]
CLASSIC_CASES += [(p, c) for p in bf.PATTERNS[1:] for c in CLASSIC if c[0] in ((64, 66), (134, 242))]
CLASSIC_CASES += [("grbg", ((65, 67), sc, 3)) for sc in (2.0, E5)]
LAYOUT_OF = {"rggb": "pitched", "grbg": "pixel_stride_2", "gbrg": "odd_window", "bggr": "packed"}


@pytest.mark.parametrize("pattern,case", CLASSIC_CASES, ids=["%s-%dx%d-s%.3g-n%d" % ((p,) + c[0] + c[1:3]) for p, c in CLASSIC_CASES])
def test_classic_pyramids_bit_identical_to_the_float32_call(rt, pattern, case):
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = case
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    assert plan.walk_plans[0] == 1 and plan.walk_plans[1] in (24, 28, 32, 36), plan.walk_plans
    for frames in (1, 3):
        _check_mosaics(rt, plan, pattern, frames, hw, "classic %s scale %.3g n %d, %d frames" % (hw, scale, n, frames), seed=n,
                       layout=LAYOUT_OF[pattern], order="rgb" if pattern == "gbrg" else "bgr")
    plan.close()


def _crops():
    hw, center, _ = odd_origin_crops()
    return [((480, 640), (288, 192), E5), (hw, center, 2.0)]


@pytest.mark.parametrize("pattern", ("rggb", "grbg"))
@pytest.mark.parametrize("which", range(2), ids=["reference-480x640", "odd-origin-270x482"])
def test_crop_layouts_bit_identical_to_the_float32_call(rt, which, pattern):
    """The union plan with its border pixels inside the walk's launch (knob 0) and behind it (knob 8), the unit + region kernels
    (knob 2), and one plan per level (knob 4 at plan creation).  The second layout's innermost crop starts at an odd row and an odd
    column: its pixels have the FRAME's parity, not the crop's."""
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import reference_levels
    hw, center, scale = _crops()[which]
    levels = reference_levels(hw, center, scale)
    if which == 1:
        assert levels[0][0] % 2 == 1 and levels[0][1] % 2 == 1
    plan = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert plan.walk_plans[0] == (2 if len(levels) >= 3 else len(levels)), plan.walk_plans
    _check_mosaics(rt, plan, pattern, 2, hw, "crops %s" % (hw,), knobs=(0, 2, 8), seed=len(levels), layout=LAYOUT_OF[pattern])
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], 3, levels)
    assert per_level.walk_plans[0] == len(levels)
    _check_mosaics(rt, per_level, pattern, 2, hw, "crops %s, one plan per level" % (hw,), knobs=(0, 8), seed=len(levels), layout=LAYOUT_OF[pattern])
    plan.close()
    per_level.close()


def test_against_the_oracle_on_the_converted_frame(rt):
    """Directly, not through the float32 path: so.classic_pyramid of the restatement's frame, within the zoom's rounding bound (the
    statement of test_rgb_nv12.test_against_the_oracle_on_the_converted_frame)."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, scale, n = (136, 240), 2.0, 4
    s = bf.spec("pitched", 2, hw[0], hw[1])
    m = bf.batch(s, seed=n)
    _, _, dev = _placed(s, m, 0xFF)
    frames = bf.truth(m, "gbrg")
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, scale, n))
    got = plan.run(dev, rgb_frame_format="bayer_gbrg")
    for f in range(2):
        want = so.classic_pyramid(frames[f], scale, n)
        for l in range(n):
            assert_close(got.level(l)[f:f + 1].cpu().numpy(), want[l], 1e-5, scale=255.0, what="gbrg frame %d level %d" % (f, l),
                         bound=eb.zoom(want[l]))
    plan.close()


def test_frame_offsets_past_2_31(rt):
    """Two 64 x 66 mosaics 2^31 + 4099 bytes apart inside one uninitialised 2.2 GiB allocation (_dev form): frame 1's addresses need
    the 64-bit frame term on every route -- a 32-bit one would read frame 0's."""
    import torch
    from pysilent_amd._lib import TUNE_PYRAMID
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (64, 66)
    stride, row = (1 << 31) + 4099, hw[1] + 6
    span = stride + (hw[0] - 1) * row + hw[1]
    free, _ = torch.cuda.mem_get_info(0)
    if free < span + (1 << 28):
        pytest.skip("not enough free device memory for a 2.2 GiB allocation")
    big = torch.empty(span + 16, dtype=torch.uint8, device="cuda:0")
    view = torch.as_strided(big, (2,) + hw, (stride, row, 1), 3)
    m = bf.batch(bf.spec("packed", 2, hw[0], hw[1]), seed=3)
    assert not np.array_equal(m[0], m[1])
    view.copy_(_t(m).cuda(0))
    assert view[1].data_ptr() - view[0].data_ptr() == stride
    f32 = _t(bf.truth(m, "bggr")).cuda(0)
    _same(rt.bayer_to_rgb(view, hw, "bayer_bggr"), f32, "frame_stride 2^31 + 4099, conversion")
    plan = rt.PyramidPlan(hw[0], hw[1], 3, classic_levels(hw, 2.0, 3))
    assert plan.walk_plans == (1, 36)
    for knob in (0, 2):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same(plan.run(view, rgb_frame_format="bayer_bggr"), plan.run(f32), "frame_stride 2^31 + 4099, PYRAMID knob %d" % knob)
    plan.close()
    del view, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals

def test_refusals_of_the_wrapper(rt):
    """The view passes as it is; the C entry point's own refusals arrive as ValueError with its text."""
    import torch
    from pysilent_amd import _lib
    m = bf.batch(bf.spec("packed", 2, 40, 48))
    dm = _t(m).cuda(0)
    B = dict(rgb_frame_format="bayer_rggb")
    plan = rt.PyramidPlan(40, 48, 3, [(0, 0, 40, 48, 40, 48, 40, 48), (0, 0, 40, 48, 20, 24, 20, 24)])
    for bad, text in ((dm.to(torch.float32), "uint8"), (dm[:, :38], r"must be \[n, 40, 48\]"), (dm.cpu(), "uint8"), ((dm, dm), "must either be"),
                      (dm[:, :1].expand(2, 40, 48), "overlap")):
        with pytest.raises((ValueError, TypeError), match=text):
            plan.run(bad, **B)
    with pytest.raises(ValueError, match="rgb_frame_format='bayer_rggb' does not combine with rgb_frame_dtype='uint8'"):
        plan.run(dm, rgb_frame_dtype="uint8", **B)
    with pytest.raises(ValueError, match="does not combine with nv12_range='full'"):
        plan.run(dm, nv12_range="full", **B)
    gray = rt.PyramidPlan(40, 48, 1, [(0, 0, 40, 48, 40, 48, 40, 48)])
    with pytest.raises(ValueError, match="rgb_frame_format='bayer_rggb' is for mode 'rgb'"):
        gray.run(dm, **B)
    lib, ctx = _lib.load(), plan.ctx
    out = torch.empty(2 * plan.frame_px * 3, dtype=torch.float32, device="cuda:0")
    optr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = rt.bayer_frames_of(dm, (40, 48), "bayer_rggb")[0]
    assert good[1:] == (1, 48, 40 * 48, 0, 0)

    def call(handle, frames, n, pyr=optr):
        ctx.check(lib.silent_pyramid_bayer_dev(ctx.handle, handle, _lib.bayer_ptr(frames), n, pyr, stream))

    def put(i, v):
        return good[:i] + (v,) + good[i + 1:]

    call(plan.handle, good, 2)
    for args, text in (((plan.handle, put(4, 4), 2), "silent_pyramid_bayer: pattern must be 0 .. 3"),
                       ((plan.handle, put(5, 2), 2), "silent_pyramid_bayer: order must be 0"),
                       ((plan.handle, put(1, 0), 2), "silent_pyramid_bayer: pixel_stride is below 1"),
                       ((plan.handle, put(2, 47), 2), "silent_pyramid_bayer: row_stride is below"),
                       ((plan.handle, put(3, 40 * 48 - 1), 2), "silent_pyramid_bayer: frame_stride is below"),
                       ((plan.handle, good, 0), "silent_pyramid_bayer: n_frames must be >= 1"),
                       ((plan.handle, good, 2, None), "silent_pyramid_bayer: NULL pointer"),
                       ((gray.handle, good, 2), "silent_pyramid_bayer: Bayer mosaics are for 3-channel plans")):
        with pytest.raises(ValueError, match=text):
            call(*args)
    torch.cuda.synchronize()
    for p in (plan, gray):
        p.close()


# ----------------------------------------------------------------------------- the pipeline

def _bytes_of(x):
    x = x.data if type(x).__name__ == "PackedPyramid" else x
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint8)


def _outputs(pipe):
    """(name, bytes) of everything the pipeline returns (pyramid, orient, line_end, value, keypoints, keypoint_counts, and with the
    attention tail its four maps and the state), whatever the dtype of a map."""
    out = pipe.outputs()
    named = []
    for k in sorted(out):
        if k == "keypoints":
            named += [("keypoints of frame %d" % f, _bytes_of(a)) for f, a in enumerate(out[k])]
        else:
            named.append((k, _bytes_of(out[k])))
    if getattr(pipe, "attention", False):
        named.append(("energy", _bytes_of(pipe.energy)))
    return named


def _same_outputs(got, want, what):
    assert [n for n, _ in got] == [n for n, _ in want], what
    for (n, g), (_, w) in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs" % (what, n)


PIPE_CASES = {"plain": ((134, 242), dict(n_levels=3), 2), "float16": ((134, 242), dict(n_levels=3, rgb_storage="float16"), 2),
              "attention": ((134, 242), dict(n_levels=3, attention=True), 3), "no-orient-map": ((134, 242), dict(n_levels=3, orient_map=False), 1), "overlap": ((134, 242), dict(n_levels=3, overlap="force"), 2),
              "reference-480x640": ((480, 640), dict(center_dimensions=(288, 192), scale=E5), 2)}


@pytest.mark.parametrize("case", list(PIPE_CASES))
def test_pipeline_on_mosaics(rt, case):
    """LineEndPipeline(mode="rgb", batch=2, selection=True, rgb_frame_format="bayer_grbg") through step and step_host against the float32
    pipeline on bayer_to_rgb(...): pyramid, orient, line_end, value, keypoints and counts (and the attention tail's maps and state after
    three steps) bit for bit, under both fills; the ingest ring holds mosaics, 1 B/px."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    hw, extra, steps = PIPE_CASES[case]
    batch, fmt = 2, "bayer_grbg"
    kw = dict(mode="rgb", batch=batch, device=0, selection=True, placement=None, **extra)
    s = bf.spec("pitched", batch, hw[0], hw[1])
    batches = [bf.batch(s, seed=11 + i) for i in range(steps)]
    ref, pipe, host = LineEndPipeline(hw, **kw), LineEndPipeline(hw, rgb_frame_format=fmt, **kw), LineEndPipeline(hw, rgb_frame_format=fmt, **kw)
    assert pipe.rgb_frame_format == fmt and pipe.rgb_frame_dtype == "float32" and pipe.frame_dtype == "float32"
    assert "bayer_grbg mosaics read in place" in pipe.launch_summary() and pipe.launch_summary().startswith(ref.launch_summary().split(", attention")[0])
    px = hw[0] * hw[1] if pipe.crop_px is None else pipe.crop_px
    assert pipe.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 12 * px + px
    for i, m in enumerate(batches):
        converted = rt.bayer_to_rgb(_t(m).cuda(0), hw, fmt)
        _same(converted, bf.truth(m, "grbg"), "bayer_to_rgb, batch %d" % i)
        ref.step(converted)
        pipe.step(_placed(s, m, bf.FILLS[i % 2])[2])
        host.step_host(bf.view(s, bf.place(s, m, bf.FILLS[1 - i % 2])) if i % 2 else m)
        for p in (ref, pipe, host):
            p.wait()
        torch.cuda.synchronize()
        want = _outputs(ref)
        _same_outputs(_outputs(pipe), want, "%s: step, batch %d" % (case, i))
        _same_outputs(_outputs(host), want, "%s: step_host, batch %d" % (case, i))
    assert {n for n, _ in want} >= {"pyramid", "line_end", "keypoint_counts", "keypoints of frame 0"}
    assert sum(int(np.frombuffer(v.tobytes(), np.int64).sum()) for n, v in want if n == "keypoint_counts") > 0
    ring = host._ingest["bayer"]["slots"]
    assert len(ring) == 2 and all(len(sl["raw"]) == 1 and sl["raw"][0].dtype == torch.uint8 and tuple(sl["raw"][0].shape) == (batch,) + hw for sl in ring)
    if case == "plain":
        # [n, H, W, 1] and contiguous mosaics are the same frames; the other order is another pipeline
        pipe.step(_t(batches[-1]).cuda(0)[..., None])
        _same_outputs(_outputs(pipe), want, "step on [n, H, W, 1]")
        synth = pipe._synthetic_frames()
        assert tuple(synth.shape) == (batch,) + hw and synth.dtype == torch.uint8 and synth.is_cuda
        for bad, text in ((converted, "uint8 GPU tensor"), (_t(batches[0]).cuda(0)[:1], "uint8 GPU tensor"), (batches[0], "uint8 GPU tensor")):
            with pytest.raises(ValueError, match=text):
                pipe.step(bad)
        with pytest.raises(ValueError, match="takes a uint8 array of shape"):
            host.step_host(batches[0].astype(np.float32))
        rgb = LineEndPipeline(hw, rgb_frame_format=fmt, nv12_order="rgb", **kw)
        ref.step(rt.bayer_to_rgb(_t(batches[0]).cuda(0), hw, fmt, "rgb"))
        rgb.step(_t(batches[0]).cuda(0))
        _same_outputs(_outputs(rgb), _outputs(ref), "nv12_order='rgb'")
        rgb.close()
    for p in (ref, pipe, host):
        p.close()
