"""Strided uint16 frames read in place (silent_*_view16; PyramidPlan.run / gray_pass / gray_keypoints and LineEndPipeline with
frame_dtype="uint16", frame_layout="strided") on the GPU.  A view changes WHERE a pixel's two bytes lie, never what is done with them,
so there is no tolerance: the oracle is the packed *_u16 path of the same build on the compacted pixels, compared as integer patterns
-- every element, every level, every frame.

Views: the valid part of a pitched [4, H * 3 / 2, 384] surface (P010 luma); x[..., 1] of a 4-channel uint16 batch; every second
element of a row; a window at the odd pixel offset (7, 5) of [4, 163, 389] frames; a view that is packed.  Each is built on the host
inside a parent whose other elements are 0x0000 and then 0xFFFF, uploaded whole and sliced on the device: an element read that is
not the view's changes an output.  Every view is legal for the ABI (even address, even strides, inside its allocation).  Frames:
tests/plan_geometry.py's 150 x 316 and 149 x 317, batch 4."""
import ctypes as C

import numpy as np
import pytest

import plan_geometry as pg
from test_gray_strided import KS, N, _compare, _consts, _plans, _same

pytestmark = pytest.mark.gpu

FRAMES_HW = (pg.FA, pg.FB)
FULL = 65535.0


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


_PIXELS = {}


def _pixels(hw):
    """The pixels every view of a frame size carries: ([4, H, W] uint16 on the host, the same packed on the device), made once."""
    import torch
    if hw not in _PIXELS:
        a = np.random.default_rng(7160 + 3 * hw[1]).integers(0, 65536, (N, hw[0], hw[1])).astype(np.uint16)
        a[0, :2, :3] = 0
        a[1, -2:, -3:] = 65535                                # both ends of the range, in the corners the mirror extension reads twice
        assert (a >= 32768).any() and ((a & 0xff) != (a >> 8)).any()
        a.setflags(write=False)
        _PIXELS[hw] = (a, torch.from_numpy(np.array(a)).cuda(0))
    return _PIXELS[hw]


# name -> (parent shape, index of the view inside the parent)
def _layouts(hw):
    H, W = hw
    return {"pitched": ((N, H * 3 // 2, 384), np.s_[:, :H, :W]),
            "channel_1_of_4": ((N, H, W, 4), np.s_[..., 1]),
            "every_second_element": ((N, H, 2 * W), np.s_[:, :, ::2]),
            "window": ((N, 163, 389), np.s_[:, 7:7 + H, 5:5 + W]),
            "packed": ((N, H, W), np.s_[:])}


VIEW_NAMES = ["pitched", "channel_1_of_4", "every_second_element", "window", "packed"]


def _view(name, hw, fill):
    """The view `name` of the pixels of `hw` on the device, every other element of its parent `fill`."""
    import torch
    shape, index = _layouts(hw)[name]
    parent = np.full(shape, fill, np.uint16)
    parent[index] = _pixels(hw)[0]
    v = torch.from_numpy(parent).cuda(0)[index]
    assert v.dtype == torch.uint16 and tuple(v.shape) == (N,) + hw and v.is_contiguous() == (name == "packed"), name
    assert v.data_ptr() % 2 == 0 and all(s > 0 for s in v.stride())
    return v


def _kind(strided):
    return dict(frame_dtype="uint16", **({"frame_layout": "strided"} if strided else {}))


def _keypoints(plan, frames, K, kind):
    """silent_gray_keypoints_u16 / _view16 _dev through the plan's operand: maps, the value maps, rows and counts."""
    from pysilent_amd import _lib
    cs_k, bank = _consts(K)
    op = plan._frames(frames, **kind)
    n, px = op.n_frames, plan.frame_px
    (pyr, pp), (cso, cp), (endo, ep), (value, vp), (peak, kp) = [op.empty(n * px * ch) for ch in (1, 1, K, 1, 1)]
    idx, iptr = op.empty((n, px, 4), np.int64)
    counts, cptr = op.empty(n, np.int64)
    reg = (_lib.Extent * len(plan.extents))(*[_lib.Extent(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents])
    op.call(plan._entry("gray_keypoints", "uint16", 1, kind.get("frame_layout", "packed")), plan.handle, op.ptr, n,
            C.c_void_p(cs_k.ctypes.data), C.c_void_p(bank.ctypes.data), K, FULL, pp, cp, ep, 2, 1, 0.1, reg, vp, kp, iptr, px, cptr)
    return pyr, cso, endo, value, peak, idx, counts


def _outputs(rt, plan, frames, strided, Ks, nostream):
    """Everything a plan computes from a batch: the gray pass with float32 and float16 maps (and with the stream kernel switched off,
    SILENT_TUNE_GRAY bit 4, where the plan streams), PyramidPlan.run on both pyramid routes, and the keypoint pass."""
    from pysilent_amd import _lib
    kind, out = _kind(strided), {}
    if not strided:
        frames = frames[..., None]                            # (the packed layout takes [n, H, W, 1])
    for K in Ks:
        cs_k, end_k = _consts(K)
        for knob in (0, 16) if nostream else (0,):
            with rt.tuning(_lib.TUNE_GRAY, knob):
                for st in ("float32", "float16"):
                    for m, t in zip(("pyramid", "cs", "end"), plan.gray_pass(frames, cs_k, end_k, FULL, storage=st, **kind)):
                        out["K%d gray knob %d %s %s" % (K, knob, st, m)] = t.data
                out["K%d gray knob %d keypoints" % (K, knob)] = _keypoints(plan, frames, K, kind)
    for knob in (0, 1):      # pyramid_stream_kernel where the plan streams / pyramid_unit_kernel + pyramid_region_kernel
        with rt.tuning(_lib.TUNE_PYRAMID, knob):
            out["run, PYRAMID knob %d" % knob] = plan.run(frames, **kind).data
    return out


# ----------------------------------------------------------------------------- 1. every view, every path

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("name", VIEW_NAMES)
def test_views_bit_identical_to_the_packed_path_and_blind_to_the_elements_around(rt, name, hw):
    n = 0
    for tag, plan, Ks, nostream in _plans(rt, hw):
        want = _outputs(rt, plan, _pixels(hw)[1], False, Ks, nostream)                 # packed *_u16 on the compacted pixels
        for fill in (0x0000, 0xFFFF):
            got = _outputs(rt, plan, _view(name, hw, fill), True, Ks, nostream)
            n += _compare(got, want, "%s %dx%d %s, parent filled 0x%04X" % (name, hw[0], hw[1], tag, fill))
        plan.close()
    print("%s %dx%d: %d elements bit-identical" % (name, hw[0], hw[1], n))


def test_view_arguments(rt):
    hw = pg.FA
    plan = _plans(rt, hw)[0][1]
    view = _view("window", hw, 0xFFFF)
    want = plan.run(_pixels(hw)[1][..., None], frame_dtype="uint16")
    _same(plan.run(view[..., None], frame_dtype="uint16", frame_layout="strided").data, want.data, "[n, H, W, 1] view")
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(view[:, :-1], frame_dtype="uint16", frame_layout="strided")
    with pytest.raises(ValueError, match="positive"):
        plan.run(view[:1].expand(N, hw[0], hw[1]), frame_dtype="uint16", frame_layout="strided")        # a broadcast: frame stride 0
    with pytest.raises(ValueError, match="contiguous"):       # the packed layout still asks for a contiguous tensor
        plan.run(view[..., None], frame_dtype="uint16")
    with pytest.raises(ValueError, match="uint8"):            # a uint8 plan call does not take a uint16 view
        plan.run(view, frame_dtype="uint8", frame_layout="strided")
    plan.close()


# ----------------------------------------------------------------------------- 2. the pipeline

def _pipe(hw, K, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    return LineEndPipeline(hw, mode="gray", n_levels=3, n_orient=K, batch=N, device=0, frame_dtype="uint16", clip_hi=FULL, **kw)


def _maps(out):
    return {k: out[k].data.clone() for k in ("pyramid", "cs", "end")}


@pytest.mark.parametrize("name,hw,K", [("pitched", pg.FA, 4), ("channel_1_of_4", pg.FB, 8), ("window", pg.FB, 3)],
                         ids=["pitched-150x316-K4", "channel_1_of_4-149x317-K8", "window-149x317-K3"])
def test_pipeline_steps_on_strided_uint16_views(rt, name, hw, K):
    """frame_layout="strided" in step, overlap="force" (the two `parts` on two streams), storage="float16" and keypoints=True gives
    what the packed uint16 pipeline gives on the compacted batch."""
    import torch
    px, view = _pixels(hw)[1][..., None], _view(name, hw, 0xFFFF)
    ref = _pipe(hw, K)
    ref.step(px)
    want = _maps(ref.outputs())
    base = _pipe(hw, K, frame_layout="strided")
    assert base.frame_layout == "strided" and "uint16 frames" in base.launch_summary() and "strided view" in base.launch_summary()
    for frames, what in ((view, "the view"), (px, "a packed tensor"), (_view(name, hw, 0x0000), "the view in a zero parent")):
        base.step(frames)
        for k, w in want.items():
            _same(base.outputs()[k].data, w, "step on %s: %s" % (what, k))
    with pytest.raises(ValueError, match="contiguous"):
        ref.step(view[..., None])
    with pytest.raises(ValueError, match="uint16 GPU tensor"):
        base.step(view.to(torch.float32))
    with pytest.raises(ValueError, match="uint16 GPU tensor"):
        base.step(view[:, 1:])
    base.run_pyramid(view)
    torch.cuda.synchronize()
    _same(base.pyr, want["pyramid"], "run_pyramid")

    ov = _pipe(hw, K, frame_layout="strided", overlap="force")
    for i in range(3):
        ov.step(view)
    for k, w in want.items():
        _same(ov.outputs()[k].data, w, "overlap='force': %s" % k)

    ref16, h16 = _pipe(hw, K, storage="float16"), _pipe(hw, K, frame_layout="strided", storage="float16")
    ref16.step(px), h16.step(view)
    assert h16.cs.dtype == torch.float16
    for k, w in _maps(ref16.outputs()).items():
        _same(h16.outputs()[k].data, w, "storage='float16': %s" % k)

    kw = dict(keypoints=True, selection=True, value_map=True, peak_value_map=True)
    refk, kp = _pipe(hw, K, **kw), _pipe(hw, K, frame_layout="strided", **kw)
    refk.step(px), kp.step(view)
    w, g = refk.outputs(), kp.outputs()
    for k in ("pyramid", "cs", "end", "value", "peak_value"):
        _same(g[k].data, w[k].data, "keypoints=True: %s" % k)
    assert np.array_equal(g["keypoint_counts"], w["keypoint_counts"]) and (w["keypoint_counts"] > 0).all()
    for f in range(N):
        assert np.array_equal(g["keypoints"][f], w["keypoints"][f]), "keypoint rows of frame %d" % f
    kp.step_host(np.array(_pixels(hw)[0])[..., None])         # step_host of a strided pipeline: its staging copy packs
    assert np.array_equal(kp.outputs()["keypoint_counts"], w["keypoint_counts"])
    for p in (ref, base, ov, ref16, h16, refk, kp):
        p.close()
