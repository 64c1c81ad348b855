"""Strided uint8 frames read in place (silent_*_view; PyramidPlan.run / gray_pass / gray_keypoints and LineEndPipeline with
frame_dtype="uint8", frame_layout="strided") on the GPU.  A view changes WHERE a pixel's bytes lie, never what is done with them, so there
is no tolerance: the oracle is the packed *_u8 / *_u8x3 path of the same build on ``view.contiguous()``, compared as integer patterns --
every element, every level, every frame.

Views (each for 1 and 3 channels where it applies): a region at (7, 5) of [4, 163, 389(, 3)] parents (odd pitch, odd offset); the luma of
a [4, 230, 384] surface; bgra[..., :3]; one channel of BGR (pixel stride 3); every second pixel of a [4, H, 2W] parent; every second
frame of eight; a BGR row pitch of 3W + 1 bytes (no multiple of 3); a packed view.  Every view runs twice, with every parent byte
outside the view's pixels 0x00 and then 0xFF: a byte read that is not the view's (a BGRA alpha, row padding, a neighbour's pixel) changes
an output.  Frames: tests/plan_geometry.py's 150 x 316 and 149 x 317 (two wave tiles, two tile rows, odd width), batch 4."""
import ctypes as C

import numpy as np
import pytest

import plan_geometry as pg

pytestmark = pytest.mark.gpu

FRAMES_HW = (pg.FA, pg.FB)
KS = (3, 4, 8)
N = 4


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


_PIXELS = {}


def _pixels(hw, channels):
    """The pixels every view of a frame size carries: [4, H, W, channels] uint8 on the device, computed once, never modified."""
    import torch
    key = (hw, channels)
    if key not in _PIXELS:
        a = np.random.default_rng(7100 + 3 * hw[1] + channels).integers(0, 256, (N, hw[0], hw[1], channels)).astype(np.uint8)
        a[0, :2, :3] = 0
        a[1, -2:, -3:] = 255                                  # both ends of the range, in the corners the mirror extension reads twice
        _PIXELS[key] = torch.from_numpy(a).cuda(0)
    return _PIXELS[key]


def _u8(shape, fill):
    import torch
    return torch.full(shape, fill, dtype=torch.uint8, device="cuda:0")


# name -> (channel counts, make(hw, ch, fill) -> the view, a [4, H, W, ch] uint8 GPU tensor inside a parent filled with `fill`)
def _roi(hw, ch, fill):
    return _u8((N, 163, 389, ch), fill)[:, 7:7 + hw[0], 5:5 + hw[1]]


def _luma(hw, ch, fill):
    return _u8((N, 230, 384), fill)[:, :hw[0], :hw[1], None]


def _bgra(hw, ch, fill):
    return _u8((N, hw[0], hw[1], 4), fill)[..., :3]


def _bgr_channel(hw, ch, fill):
    return _u8((N, hw[0], hw[1], 3), fill)[..., 1:2]


def _every_second_pixel(hw, ch, fill):
    return _u8((N, hw[0], 2 * hw[1], ch), fill)[:, :, ::2]


def _every_second_frame(hw, ch, fill):
    return _u8((2 * N, hw[0], hw[1], ch), fill)[::2]


def _odd_pitch_bgr(hw, ch, fill):
    import torch
    pitch = 3 * hw[1] + 1                                     # bytes: no multiple of 3, every second row starts at another phase
    return torch.as_strided(_u8((N * hw[0] * pitch,), fill), (N, hw[0], hw[1], 3), (hw[0] * pitch, pitch, 3, 1))


def _packed(hw, ch, fill):
    return _u8((N, hw[0], hw[1], ch), fill)


VIEWS = {"roi": ((1, 3), _roi), "luma": ((1,), _luma), "bgra": ((3,), _bgra), "bgr_channel": ((1,), _bgr_channel),
         "every_second_pixel": ((1, 3), _every_second_pixel), "every_second_frame": ((1, 3), _every_second_frame),
         "odd_pitch_bgr": ((3,), _odd_pitch_bgr), "packed": ((1, 3), _packed)}
VIEW_CASES = [(name, ch) for name in sorted(VIEWS) for ch in VIEWS[name][0]]
VIEW_IDS = ["%s-c%d" % vc for vc in VIEW_CASES]


def _view(name, hw, ch, fill):
    v = VIEWS[name][1](hw, ch, fill)
    assert tuple(v.shape) == (N, hw[0], hw[1], ch) and v.is_contiguous() == (name == "packed"), name
    v.copy_(_pixels(hw, ch))
    return v


def _kind(ch, strided):
    return dict(frame_dtype="uint8", frame_channels=ch, **({"frame_layout": "strided"} if strided else {}))


def _consts(K):
    from pysilent_amd.pipeline import default_constants
    c = default_constants("gray", K)
    return np.ascontiguousarray(c["cs"], np.float32), np.ascontiguousarray(c["end"], np.float32)


def _bits(a):
    import torch
    return a.contiguous().view({torch.float32: torch.int32, torch.float16: torch.int16, torch.int64: torch.int64}[a.dtype])


def _same(got, want, what):
    import torch
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, what
    bad = int((g != w).sum())
    assert bad == 0, "%s: %d of %d elements differ from the packed path; first at %d" % (what, bad, g.numel(), int(torch.nonzero((g != w).reshape(-1))[0]))
    return g.numel()


def _keypoints(rt, plan, frames, K, kind):
    """silent_gray_keypoints_u8 / _u8x3 / _view _dev through the plan's operand: maps, the value map, rows and counts."""
    from pysilent_amd import _lib
    cs_k, bank = _consts(K)
    op = plan._frames(frames, **kind)
    n, px = op.n_frames, plan.frame_px
    (pyr, pp), (cso, cp), (endo, ep), (value, vp), (peak, kp) = [op.empty(n * px * ch) for ch in (1, 1, K, 1, 1)]
    idx, iptr = op.empty((n, px, 4), np.int64)
    counts, cptr = op.empty(n, np.int64)
    reg = (_lib.Extent * len(plan.extents))(*[_lib.Extent(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents])
    op.call(plan._entry("gray_keypoints", kind["frame_dtype"], kind["frame_channels"], kind.get("frame_layout", "packed")), plan.handle, op.ptr, n,
            C.c_void_p(cs_k.ctypes.data), C.c_void_p(bank.ctypes.data), K, 255.0, pp, cp, ep, 2, 1, 0.1, reg, vp, kp, iptr, px, cptr)
    return pyr, cso, endo, value, peak, idx, counts


def _outputs(rt, plan, frames, ch, strided, Ks, nostream):
    """Everything a plan computes from a batch: the gray pass with float32 and float16 maps (and with the stream kernel switched off,
    SILENT_TUNE_GRAY bit 4, where the plan streams), PyramidPlan.run on both pyramid routes, and the keypoint pass."""
    from pysilent_amd import _lib
    kind, out = _kind(ch, strided), {}
    for K in Ks:
        cs_k, end_k = _consts(K)
        for knob in (0, 16) if nostream else (0,):
            with rt.tuning(_lib.TUNE_GRAY, knob):
                for st in ("float32", "float16"):
                    for m, t in zip(("pyramid", "cs", "end"), plan.gray_pass(frames, cs_k, end_k, 255.0, storage=st, **kind)):
                        out["K%d gray knob %d %s %s" % (K, knob, st, m)] = t.data
                out["K%d gray knob %d keypoints" % (K, knob)] = _keypoints(rt, plan, frames, K, kind)
    for knob in (0, 1):      # pyramid_stream_kernel where the plan streams / pyramid_unit_kernel + pyramid_region_kernel
        with rt.tuning(_lib.TUNE_PYRAMID, knob):
            out["run, PYRAMID knob %d" % knob] = plan.run(frames, **kind).data
    return out


def _compare(got, want, tag):
    import torch
    n = 0
    assert sorted(got) == sorted(want)
    for k in want:
        if not k.endswith("keypoints"):
            n += _same(got[k], want[k], "%s: %s" % (tag, k))
            continue
        for g, w, m in zip(got[k][:5], want[k][:5], ("pyramid", "cs", "end", "value", "peak_value")):
            n += _same(g, w, "%s: %s %s" % (tag, k, m))
        gc, wc_ = got[k][6].cpu().numpy(), want[k][6].cpu().numpy()
        assert (wc_ > 0).all() and np.array_equal(gc, wc_), "%s: %s counts %s, packed path %s" % (tag, k, gc, wc_)
        for f in range(len(wc_)):                             # rows exact (rows past counts[f] are unspecified)
            assert torch.equal(got[k][5][f, :wc_[f]], want[k][5][f, :wc_[f]]), "%s: %s keypoint rows of frame %d" % (tag, k, f)
    return n


def _plans(rt, hw):
    """(tag, plan, K's, also without the stream kernel): a streamable classic plan, a crop layout and a plan without a unit level."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    sfx = "_316" if hw == pg.FA else "_317"
    classic = rt.PyramidPlan(hw[0], hw[1], 1, classic_levels(hw, 2.0, 3), 0)
    assert classic.streamable
    out = [("classic", classic, KS, True)]
    for name in ("nested" + sfx, "no_unit" + sfx):
        assert pg.CASES[name]["frame"] == hw
        p = rt.PyramidPlan(hw[0], hw[1], 1, pg.CASES[name]["levels"], 0)
        assert not p.streamable
        out.append((name, p, KS if name.startswith("nested") else (4,), False))    # the crop layout: gray_unit_fused_kernel<3 | 4 | 8>
    return out


# ----------------------------------------------------------------------------- 1. every view, every path

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("name,ch", VIEW_CASES, ids=VIEW_IDS)
def test_views_bit_identical_to_the_packed_path_and_blind_to_the_bytes_around(rt, name, ch, hw):
    import torch
    n = 0
    for tag, plan, Ks, nostream in _plans(rt, hw):
        want = _outputs(rt, plan, _pixels(hw, ch), ch, False, Ks, nostream)            # packed *_u8 / *_u8x3 on view.contiguous()
        for fill in (0x00, 0xFF):
            view = _view(name, hw, ch, fill)
            assert torch.equal(view.contiguous(), _pixels(hw, ch))
            got = _outputs(rt, plan, view, ch, True, Ks, nostream)
            n += _compare(got, want, "%s c%d %dx%d %s, parent filled 0x%02X" % (name, ch, hw[0], hw[1], tag, fill))
        plan.close()
    print("%s c%d %dx%d: %d elements bit-identical" % (name, ch, hw[0], hw[1], n))


def test_one_channel_views_may_drop_the_channel_axis(rt):
    hw = pg.FA
    plan = _plans(rt, hw)[0][1]
    view = _view("roi", hw, 1, 0xFF)
    want = plan.run(_pixels(hw, 1), frame_dtype="uint8")
    _same(plan.run(view[..., 0], frame_dtype="uint8", frame_layout="strided").data, want.data, "[n, H, W] view")
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(view[:, :-1], frame_dtype="uint8", frame_layout="strided")
    with pytest.raises(ValueError, match="positive"):
        plan.run(view[:1].expand(N, hw[0], hw[1], 1), frame_dtype="uint8", frame_layout="strided")      # a broadcast: frame stride 0
    with pytest.raises(ValueError, match="contiguous"):       # the packed layout still asks for a contiguous tensor
        plan.run(view, frame_dtype="uint8")
    plan.close()


# ----------------------------------------------------------------------------- 2. the pipeline: step, the two parts, keypoints, float16

def _pipe(hw, K, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    return LineEndPipeline(hw, mode="gray", n_levels=3, n_orient=K, batch=N, device=0, frame_dtype="uint8", **kw)


def _maps(out):
    return {k: out[k].data.clone() for k in ("pyramid", "cs", "end")}


@pytest.mark.parametrize("name,ch,hw,K", [("roi", 1, pg.FA, 4), ("bgra", 3, pg.FB, 8), ("luma", 1, pg.FB, 3), ("odd_pitch_bgr", 3, pg.FA, 4)],
                         ids=["roi-c1-150x316-K4", "bgra-c3-149x317-K8", "luma-c1-149x317-K3", "odd_pitch_bgr-c3-150x316-K4"])
def test_pipeline_steps_on_strided_views(rt, name, ch, hw, K):
    """frame_layout="strided" in step, overlap="force" (the two `parts` on two streams), placement="auto", storage="float16" and
    keypoints=True gives what the packed uint8 pipeline gives on the compacted batch."""
    import torch
    px, view = _pixels(hw, ch), _view(name, hw, ch, 0xFF)
    ref = _pipe(hw, K, frame_channels=ch)
    ref.step(px)
    want = _maps(ref.outputs())
    base = _pipe(hw, K, frame_channels=ch, frame_layout="strided")
    assert base.frame_layout == "strided" and ref.frame_layout == "packed" and "strided view" in base.launch_summary()
    for frames, what in ((view, "the view"), (px, "a packed tensor"), (_view(name, hw, ch, 0x00), "the view in a zero parent")):
        base.step(frames)
        for k, w in want.items():
            _same(base.outputs()[k].data, w, "step on %s: %s" % (what, k))
    with pytest.raises(ValueError, match="contiguous"):
        ref.step(view)
    with pytest.raises(ValueError, match="uint8 GPU tensor"):
        base.step(view.to(torch.float32))
    with pytest.raises(ValueError, match="uint8 GPU tensor"):
        base.step(view[:, 1:])
    with pytest.raises(ValueError, match="positive"):
        base.step(view[:, :1].expand(N, hw[0], hw[1], ch))          # a broadcast: row stride 0
    base.run_pyramid(view)
    torch.cuda.synchronize()
    _same(base.pyr, want["pyramid"], "run_pyramid")

    ov = _pipe(hw, K, frame_channels=ch, frame_layout="strided", overlap="force")
    for i in range(3):
        ov.step(view)
    for k, w in want.items():
        _same(ov.outputs()[k].data, w, "overlap='force': %s" % k)

    tuned = _pipe(hw, K, frame_channels=ch, frame_layout="strided", placement="auto")
    tuned.step(view)
    assert tuned.placement_tuning is not None
    for k, w in want.items():
        _same(tuned.outputs()[k].data, w, "placement='auto': %s" % k)
    assert tuned.tune_placement(tries=2, steps=3, budget_s=0.3)["tries_ms"]      # (on the tuner's own synthetic frames: a packed view)

    ref16, h16 = _pipe(hw, K, frame_channels=ch, storage="float16"), _pipe(hw, K, frame_channels=ch, frame_layout="strided", storage="float16")
    ref16.step(px), h16.step(view)
    assert h16.cs.dtype == torch.float16
    for k, w in _maps(ref16.outputs()).items():
        _same(h16.outputs()[k].data, w, "storage='float16': %s" % k)

    kw = dict(keypoints=True, selection=True, value_map=True, peak_value_map=True, frame_channels=ch)
    refk, kp = _pipe(hw, K, **kw), _pipe(hw, K, frame_layout="strided", **kw)
    refk.step(px), kp.step(view)
    w, g = refk.outputs(), kp.outputs()
    for k in ("pyramid", "cs", "end", "value", "peak_value"):
        _same(g[k].data, w[k].data, "keypoints=True: %s" % k)
    assert np.array_equal(g["keypoint_counts"], w["keypoint_counts"]) and (w["keypoint_counts"] > 0).all()
    for f in range(N):
        assert np.array_equal(g["keypoints"][f], w["keypoints"][f]), "keypoint rows of frame %d" % f
    # step_host is unchanged: its staging copy packs
    kp.step_host(px.cpu().numpy())
    assert np.array_equal(kp.outputs()["keypoint_counts"], w["keypoint_counts"])
    for p in (ref, base, ov, tuned, ref16, h16, refk, kp):
        p.close()


# ----------------------------------------------------------------------------- 3. 64-bit byte offsets

def test_frame_stride_past_2_31(rt):
    """Two frames 2^31 + 4099 bytes apart inside one uninitialised 2.2 GiB allocation (_dev forms): frame 1's address needs the
    64-bit frame term, and 4099 makes it odd."""
    import torch
    hw, K = pg.FB, 4
    stride = (1 << 31) + 4099
    row = hw[1] + 3
    span = stride + (hw[0] - 1) * row + hw[1]
    big = torch.empty(span + 16, dtype=torch.uint8, device="cuda:0")
    view = torch.as_strided(big, (2, hw[0], hw[1], 1), (stride, row, 1, 1), 5)
    px = _pixels(hw, 1)[:2]
    view.copy_(px)
    assert view.data_ptr() == big.data_ptr() + 5 and view[1].data_ptr() - view[0].data_ptr() == stride
    for tag, plan, _, nostream in _plans(rt, hw):
        want = _outputs(rt, plan, px.contiguous(), 1, False, (K,), nostream)
        got = _outputs(rt, plan, view, 1, True, (K,), nostream)
        _compare(got, want, "frame_stride 2^31 + 4099, %s" % tag)
        plan.close()
    del view, big
    torch.cuda.empty_cache()
