"""Interleaved 3-channel uint8 frames read as they are (silent_*_u8x3; PyramidPlan.run / gray_pass / gray_keypoints and
LineEndPipeline with frame_dtype="uint8", frame_channels=3) on the GPU.  Each frame pixel enters the arithmetic as
v = (float)(b0 + b1 + b2) * float32(1/3), formed in registers at the load -- the sum is exact, the multiply is one rounding -- so
there is no tolerance: the oracle of everything but the last test is the float32-frame path of the same build on the frame of v
values (computed in numpy float32 and first shown to be silent_value_from_color_dev's output bit for bit), compared as integer
patterns -- every element, every level, every frame.  The last test ties the new path to the C oracle directly.

Frames: three seeded uint8 noise frames with independent channels over 0 .. 255 and one structured frame, on the 150 x 316 and
149 x 317 frames of tests/plan_geometry.py (two 56-column wave tiles, two tile rows, two region blocks; a 317 x 3 = 951-byte row
makes every second row start odd, and the odd frame stride puts frames 1 and 3 of that batch at odd addresses)."""
import math

import numpy as np
import pytest

import err_bound as eb
import plan_geometry as pg
from conftest import assert_close, structured_frame

pytestmark = pytest.mark.gpu

E5 = float(math.e) ** .5
FRAMES_HW = (pg.FA, pg.FB)
KS = (3, 4, 8)
U8X3 = dict(frame_dtype="uint8", frame_channels=3)
THIRD = np.float32(1.0) / np.float32(3.0)


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def value_of(rgb8):
    """v = ((f0 + f1) + f2) * float32(1/3) in numpy float32: [..., 3] uint8 -> [..., 1] float32."""
    f = rgb8.astype(np.float32)
    v = ((f[..., 0] + f[..., 1]) + f[..., 2]) * THIRD
    assert v.dtype == np.float32
    return np.ascontiguousarray(v[..., None])


_BATCH = {}


def _batch(hw):
    """(uint8 colour frames [4, H, W, 3], their value frames [4, H, W, 1] float32): computed once, never modified."""
    if hw not in _BATCH:
        rgb8 = np.stack([np.random.default_rng(9900 + 13 * hw[1] + i).integers(0, 256, (hw[0], hw[1], 3)).astype(np.uint8) for i in range(3)]
                        + [np.clip(structured_frame(37, hw[0], hw[1], 3), 0, 255).astype(np.uint8)])
        assert rgb8.dtype == np.uint8 and rgb8.shape == (4, hw[0], hw[1], 3)
        for ch in range(3):
            c = rgb8[..., ch]
            assert (c == 0).any() and (c == 255).any() and (c >= 128).any(), ch
        assert not np.array_equal(rgb8[..., 0], rgb8[..., 1]) and not np.array_equal(rgb8[..., 1], rgb8[..., 2])
        # channel sums on which a division by 3 would give other bits than the multiply by float32(1/3)
        s = rgb8.astype(np.int32).sum(axis=-1).astype(np.float32)
        differ = (s * THIRD).view(np.int32) != (s / np.float32(3)).view(np.int32)
        assert differ.mean() > 0.2, differ.mean()
        v = value_of(rgb8)
        for a in (rgb8, v):
            a.setflags(write=False)
        _BATCH[hw] = (rgb8, v)
    return _BATCH[hw]


def _t(a):
    """A torch CPU tensor holding a copy of ``a`` (the shared batches are read-only)."""
    import torch
    return torch.from_numpy(np.array(a))


def _consts(K):
    from pysilent_amd.pipeline import default_constants
    c = default_constants("gray", K)
    return np.ascontiguousarray(c["cs"], np.float32), np.ascontiguousarray(c["end"], np.float32)


def _f32_bits(a):
    a = np.ascontiguousarray(a, np.float32)
    assert not np.isnan(a).any()                  # (finite frames: no NaN anywhere, so the patterns are compared as they are)
    return a.view(np.int32)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same_f32(got, want, what):
    got, want = _np(got), _np(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    gb, wb = _f32_bits(got), _f32_bits(want)
    bad = int((gb != wb).sum())
    assert bad == 0, "%s: %d of %d elements differ from the float32-frame path; first at %d" % (what, bad, gb.size, int(np.flatnonzero(gb != wb)[0]))


def _same_f16(got, want, what):
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape, what
    assert not np.isnan(want).any()
    bad = int((got.view(np.uint16) != want.view(np.uint16)).sum())
    assert bad == 0, "%s: %d of %d float16 patterns differ from silent_gray_pass_h's" % (what, bad, got.size)


def _levels(family, hw):
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    if family in ("ratio2_3", "ratio2_3_nostream"):
        return classic_levels(hw, 2.0, 3), True            # 2 general levels: gray_stream_kernel<K, 4, 0>
    if family == "ratio2_6":
        return classic_levels(hw, 2.0, 6), True            # 5 general levels: <K, 7, 0>
    if family == "sqrt2_4":
        return classic_levels(hw, 2.0 ** .5, 4), True      # five rows of the first level in flight: slot layout 1, <K, 7, 1>
    if family == "one_level":
        return classic_levels(hw, 2.0, 1), False           # no general level: the unit-fused kernel alone
    if family == "reference_crop":
        return reference_levels(hw, (48, 32), E5), False   # nested centre crops: region + unit-fused + filter kernels
    raise KeyError(family)


FAMILIES = ["ratio2_3", "ratio2_6", "sqrt2_4", "one_level", "reference_crop", "ratio2_3_nostream"]


class _Knobs(object):
    """*_nostream: the stream kernel of the gray pass switched off (SILENT_TUNE_GRAY bit 4): region + unit-fused + filter kernels."""

    def __init__(self, rt, family):
        self.rt, self.on = rt, family.endswith("_nostream")

    def __enter__(self):
        from pysilent_amd import _lib
        if self.on:
            self.g = self.rt.tuning(_lib.TUNE_GRAY, 16)
            self.g.__enter__()

    def __exit__(self, *exc):
        if self.on:
            self.g.__exit__(*exc)


def _check_plan(rt, plan, rgb8, v, K, knobs, tag):
    """gray_pass (float32 and float16 maps) and run (stream kernel, and unit + region kernels) on colour uint8 frames against the same
    calls on the frame of values.  Returns the number of elements compared."""
    from pysilent_amd import _lib
    cs_k, end_k = _consts(K)
    n = 0
    with knobs:
        want = plan.gray_pass(v, cs_k, end_k, 255.0)
        got = plan.gray_pass(rgb8, cs_k, end_k, 255.0, **U8X3)
        want16 = plan.gray_pass(v, cs_k, end_k, 255.0, storage="float16")
        got16 = plan.gray_pass(rgb8, cs_k, end_k, 255.0, storage="float16", **U8X3)
    for g, w, m in zip(got, want, ("pyramid", "cs", "end")):
        _same_f32(g.data, w.data, "%s K=%d gray_pass %s" % (tag, K, m))
        n += g.data.size
    _same_f32(got16[0].data, want16[0].data, "%s K=%d float16-map pass: pyramid" % (tag, K))
    for g, w, m in zip(got16[1:], want16[1:], ("cs", "end")):
        _same_f16(g.data, w.data, "%s K=%d float16 %s" % (tag, K, m))
        n += g.data.size
    for knob in (0, 1):      # pyramid_stream_kernel where the plan streams / pyramid_unit_kernel + pyramid_region_kernel
        with rt.tuning(_lib.TUNE_PYRAMID, knob):
            w = plan.run(v)
            g = plan.run(rgb8, **U8X3)
        _same_f32(g.data, w.data, "%s run(), PYRAMID knob %d" % (tag, knob))
        _same_f32(g.data, want[0].data, "%s run() vs the gray pass's pyramid, PYRAMID knob %d" % (tag, knob))
        n += g.data.size
    return n


# ----------------------------------------------------------------------------- 0. the expected input

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
def test_expected_value_frame_is_silent_value_from_color_on_the_widened_frames(rt, hw):
    """numpy's ((f0 + f1) + f2) * float32(1/3) equals silent_value_from_color_dev on the widened colour frames, bit for bit: the
    oracle input of every test below is what the library's own a-8 kernel makes of the frames."""
    rgb8, v = _batch(hw)
    got = rt.value_from_color(_t(rgb8.astype(np.float32)).cuda(0))
    assert tuple(got.shape) == v.shape
    _same_f32(got, v, "value_from_color %dx%d" % hw)


# ----------------------------------------------------------------------------- 1. kernel families

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", FAMILIES)
def test_kernel_families_bit_identical_to_the_float32_frame_path(rt, family, hw):
    rgb8, v = _batch(hw)
    levels, streamable = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    assert plan.streamable == streamable, (family, hw)
    n = 0
    for K in KS:
        n += _check_plan(rt, plan, rgb8, v, K, _Knobs(rt, family), "%s %dx%d" % (family, hw[0], hw[1]))
    print("%s %dx%d: %d elements bit-identical" % (family, hw[0], hw[1], n))
    plan.close()


# ----------------------------------------------------------------------------- 2. unusual geometry

@pytest.mark.parametrize("name", sorted(pg.CASES))
def test_plan_geometry_cases_bit_identical(rt, name):
    """Sub-windows with src_x0 % 4 = 0 .. 3, unit canvases, two unit levels, no unit level, upsampling, degenerate axes, crop
    layouts (tests/plan_geometry.py: every case, as a single-channel plan), K = 4."""
    case = pg.CASES[name]
    hw = case["frame"]
    rgb8, v = _batch(hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, case["levels"], 0)
    assert plan.streamable == pg.ROUTES[name][0][0], name
    _check_plan(rt, plan, rgb8, v, 4, _Knobs(rt, ""), name)
    if plan.streamable:
        _check_plan(rt, plan, rgb8, v, 4, _Knobs(rt, "_nostream"), name + " (no stream kernel)")
    plan.close()


# ----------------------------------------------------------------------------- 3. misaligned base

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", ["ratio2_3", "ratio2_3_nostream", "reference_crop"])
def test_misaligned_base_pointer(rt, family, hw):
    """The frames pointer has no alignment requirement: the same batch at byte offsets 0 .. 3 of a larger device buffer gives the
    same outputs (149 x 317 x 3 also makes every second row start odd)."""
    import torch
    from pysilent_amd import _lib
    rgb8, v = _batch(hw)
    levels, _ = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    cs_k, end_k = _consts(4)
    nbytes = rgb8.size
    big = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert big.data_ptr() % 4 == 0
    flat = _t(rgb8.reshape(-1))
    outs = []
    for off in (0, 1, 2, 3):
        big.fill_(0xA5)
        view = big[off:off + nbytes]
        view.copy_(flat)
        frames = view.view(rgb8.shape)
        assert frames.is_contiguous() and frames.data_ptr() % 4 == off
        with _Knobs(rt, family):
            p, c, e = plan.gray_pass(frames, cs_k, end_k, 255.0, **U8X3)
            runs = []
            for knob in (0, 1):
                with rt.tuning(_lib.TUNE_PYRAMID, knob):
                    runs.append(plan.run(frames, **U8X3).data.cpu().numpy())
        torch.cuda.synchronize()
        outs.append([p.data.cpu().numpy(), c.data.cpu().numpy(), e.data.cpu().numpy()] + runs)
    with _Knobs(rt, family):
        want = plan.gray_pass(v, cs_k, end_k, 255.0)
    for off in (0, 1, 2, 3):
        for g, w, m in zip(outs[off][:3], want, ("pyramid", "cs", "end")):
            _same_f32(g, w.data, "%s offset %d %s" % (family, off, m))
        for knob in (0, 1):
            _same_f32(outs[off][3 + knob], want[0].data, "%s offset %d run(), PYRAMID knob %d" % (family, off, knob))
    plan.close()


# ----------------------------------------------------------------------------- 4. the C ABI directly

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", ["ratio2_3", "reference_crop"])
def test_c_abi_host_forms_dev_forms_parts_and_float16_maps(rt, family, hw):
    """silent_gray_pass_u8x3 / silent_pyramid_u8x3 on a uint8 ndarray against their _dev forms on a device copy (parts = 3, and
    parts = 1 then 2 on poisoned buffers), maps_f16 = 0 against silent_gray_pass and maps_f16 = 1 against the uint16 patterns
    silent_gray_pass_h stores for the frame of values; NULL cs_out / end_out; the status codes."""
    import torch
    from pysilent_amd import _lib
    lib = _lib.load()
    rgb8, v = _batch(hw)
    levels, _ = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    K = 4
    cs_k, end_k = _consts(K)
    n, px = rgb8.shape[0], plan.frame_px
    h, c = plan.ctx.handle, plan.ctx.check
    want = plan.gray_pass(v, cs_k, end_k, 255.0)
    want16 = plan.gray_pass(v, cs_k, end_k, 255.0, storage="float16")
    frames_h = np.ascontiguousarray(rgb8)
    frames_d = _t(frames_h).cuda(0)
    fh, fd = _lib.byte_ptr(frames_h.ctypes.data), _lib.byte_ptr(frames_d.data_ptr())
    s = torch.cuda.current_stream().cuda_stream

    for f16 in (0, 1):
        dt, tdt = (np.float16, torch.float16) if f16 else (np.float32, torch.float32)
        same = _same_f16 if f16 else _same_f32
        ref = want16 if f16 else want
        # host form, then with one output NULL
        pyr, cs, end = np.full(n * px, -7.0, np.float32), np.full(n * px, 3.0, dt), np.full(n * px * K, 3.0, dt)
        c(lib.silent_gray_pass_u8x3(h, plan.handle, fh, n, cs_k.ctypes.data, end_k.ctypes.data, K, 255.0,
                                    pyr.ctypes.data, cs.ctypes.data, end.ctypes.data, f16))
        _same_f32(pyr, ref[0].data, "host form pyramid (maps_f16 = %d)" % f16)
        same(cs, ref[1].data, "host form cs (maps_f16 = %d)" % f16)
        same(end, ref[2].data, "host form end (maps_f16 = %d)" % f16)
        for drop in ("cs", "end"):
            p2, c2, e2 = np.full(n * px, -7.0, np.float32), np.full(n * px, 3.0, dt), np.full(n * px * K, 3.0, dt)
            c(lib.silent_gray_pass_u8x3(h, plan.handle, fh, n, cs_k.ctypes.data, end_k.ctypes.data, K, 255.0,
                                        p2.ctypes.data, None if drop == "cs" else c2.ctypes.data, None if drop == "end" else e2.ctypes.data, f16))
            _same_f32(p2, pyr, "NULL %s_out: pyramid" % drop)
            same(e2 if drop == "cs" else c2, end if drop == "cs" else cs, "NULL %s_out: the other map" % drop)

        def run(parts_seq):
            p = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
            cm = torch.full((n * px,), 3.0, dtype=tdt, device="cuda:0")
            em = torch.full((n * px * K,), 3.0, dtype=tdt, device="cuda:0")
            for parts in parts_seq:
                c(lib.silent_gray_pass_u8x3_dev(h, plan.handle, fd, n, cs_k.ctypes.data, end_k.ctypes.data, K,
                                                255.0, p.data_ptr(), cm.data_ptr(), em.data_ptr(), f16, parts, s))
            torch.cuda.synchronize()
            return p.cpu().numpy(), cm.cpu().numpy(), em.cpu().numpy()

        whole, halves = run([3]), run([1, 2])
        _same_f32(whole[0], pyr, "_dev form pyramid")
        _same_f32(halves[0], pyr, "parts 1 + 2 pyramid")
        for a, b, r, m in zip(whole[1:], halves[1:], (cs, end), ("cs", "end")):
            same(a, r, "_dev form %s differs from the host form (maps_f16 = %d)" % (m, f16))
            same(b, r, "parts 1 + 2 %s differ from parts = 3 (maps_f16 = %d)" % (m, f16))
    # silent_pyramid_u8x3: host form against the _dev form against the gray pass's pyramid
    ph = np.full(n * px, -7.0, np.float32)
    c(lib.silent_pyramid_u8x3(h, plan.handle, fh, n, ph.ctypes.data))
    pd = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
    c(lib.silent_pyramid_u8x3_dev(h, plan.handle, fd, n, pd.data_ptr(), s))
    torch.cuda.synchronize()
    _same_f32(ph, want[0].data, "silent_pyramid_u8x3")
    _same_f32(pd.cpu().numpy(), ph, "silent_pyramid_u8x3_dev")

    # ---- status codes
    INVALID, UNSUPPORTED = _lib.SILENT_E_INVALID, _lib.SILENT_E_UNSUPPORTED
    ck, ek = cs_k.ctypes.data, end_k.ctypes.data
    pd_, cd_, ed_ = (torch.empty(n * px * m, dtype=torch.float32, device="cuda:0") for m in (1, 1, K))
    pp, cp, ep = pd_.data_ptr(), cd_.data_ptr(), ed_.data_ptr()

    def gp(plan_h, frames, n_, k, pyr_p, cs_p, end_p, parts=3):
        return lib.silent_gray_pass_u8x3_dev(h, plan_h, frames, n_, ck, ek, k, 255.0, pyr_p, cs_p, end_p, 0, parts, s)

    def gph(plan_h, frames, n_, k, pyr_p, cs_p, end_p):
        return lib.silent_gray_pass_u8x3(h, plan_h, frames, n_, ck, ek, k, 255.0, pyr_p, cs_p, end_p, 0)

    hp, hc, he = ph.ctypes.data, np.empty(n * px, np.float32), np.empty(n * px * K, np.float32)
    assert gp(None, fd, n, K, pp, cp, ep) == INVALID and gp(plan.handle, None, n, K, pp, cp, ep) == INVALID
    assert gp(plan.handle, fd, n, K, None, cp, ep) == INVALID and gp(plan.handle, fd, n, K, pp, None, None) == INVALID
    assert gp(plan.handle, fd, 0, K, pp, cp, ep) == INVALID and gp(plan.handle, fd, n, K, pp, cp, ep, parts=0) == INVALID
    assert gp(plan.handle, fd, n, 5, pp, cp, ep) == UNSUPPORTED
    assert gph(None, fh, n, K, hp, hc.ctypes.data, he.ctypes.data) == INVALID and gph(plan.handle, None, n, K, hp, hc.ctypes.data, he.ctypes.data) == INVALID
    assert gph(plan.handle, fh, n, K, None, hc.ctypes.data, he.ctypes.data) == INVALID and gph(plan.handle, fh, n, K, hp, None, None) == INVALID
    assert gph(plan.handle, fh, 0, K, hp, hc.ctypes.data, he.ctypes.data) == INVALID
    assert gph(plan.handle, fh, n, 5, hp, hc.ctypes.data, he.ctypes.data) == UNSUPPORTED
    assert lib.silent_pyramid_u8x3(h, None, fh, n, hp) == INVALID and lib.silent_pyramid_u8x3(h, plan.handle, None, n, hp) == INVALID
    assert lib.silent_pyramid_u8x3(h, plan.handle, fh, n, None) == INVALID and lib.silent_pyramid_u8x3(h, plan.handle, fh, 0, hp) == INVALID
    assert lib.silent_pyramid_u8x3_dev(h, None, fd, n, pp, s) == INVALID and lib.silent_pyramid_u8x3_dev(h, plan.handle, None, n, pp, s) == INVALID
    assert lib.silent_pyramid_u8x3_dev(h, plan.handle, fd, n, None, s) == INVALID and lib.silent_pyramid_u8x3_dev(h, plan.handle, fd, 0, pp, s) == INVALID
    regions = [(max(eh // 2, 1), max(ew // 2, 1)) for eh, ew in plan.extents]
    reg = (_lib.Extent * len(regions))(*[_lib.Extent(a, b) for a, b in regions])
    idx = torch.empty((n, px, 4), dtype=torch.int64, device="cuda:0")
    counts = torch.empty(n, dtype=torch.int64, device="cuda:0")

    def kp(plan_h, frames, n_, k):
        return lib.silent_gray_keypoints_u8x3_dev(h, plan_h, frames, n_, ck, ek, k, 255.0, pp, cp, ep, 2, 1, 0.1, reg, None, None,
                                                  idx.data_ptr(), px, counts.data_ptr(), s)

    assert kp(None, fd, n, K) == INVALID and kp(plan.handle, None, n, K) == INVALID and kp(plan.handle, fd, 0, K) == INVALID
    assert kp(plan.handle, fd, n, 5) == UNSUPPORTED
    # a plan of another context
    other_ctx = rt.Context(0)
    other_plan = C_plan(_lib, other_ctx, hw, levels)
    assert gp(other_plan, fd, n, K, pp, cp, ep) == INVALID and kp(other_plan, fd, n, K) == INVALID
    assert lib.silent_pyramid_u8x3_dev(h, other_plan, fd, n, pp, s) == INVALID
    lib.silent_pyramid_plan_destroy(other_plan)
    other_ctx.close()
    # a float64 plan, a 3-channel plan: refused by the new entry points, and the *_u8 ones still refuse the 3-channel plan
    p64 = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0, accumulation="float64")
    p3 = rt.PyramidPlan(hw[0], hw[1], 3, levels, 0)
    for bad in (p64, p3):
        assert lib.silent_pyramid_u8x3(h, bad.handle, fh, n, hp) == UNSUPPORTED
        assert lib.silent_pyramid_u8x3_dev(h, bad.handle, fd, n, pp, s) == UNSUPPORTED
        assert gph(bad.handle, fh, n, K, hp, None, None) == UNSUPPORTED
        assert gp(bad.handle, fd, n, K, pp, cp, ep) == UNSUPPORTED
        assert kp(bad.handle, fd, n, K) == UNSUPPORTED
        bad_h = bad.handle
        assert lib.silent_pyramid_u8(h, bad_h, fh, n, hp) == UNSUPPORTED
        assert lib.silent_gray_pass_u8(h, bad_h, fh, n, ck, ek, K, 255.0, hp, None, None, 0) == UNSUPPORTED
        bad.close()
    with pytest.raises(ValueError, match="frame_channels"):
        rt.PyramidPlan(hw[0], hw[1], 1, levels, 0, accumulation="float64").run(rgb8, **U8X3)
    with pytest.raises(ValueError, match="frame_channels"):
        plan.gray_pass(rgb8, cs_k, end_k, 255.0, frame_channels=3)                      # (frame_dtype left at "float32")
    with pytest.raises(ValueError, match="uint8"):
        plan.gray_pass(rgb8.astype(np.float32), cs_k, end_k, 255.0, **U8X3)            # nothing is converted silently
    with pytest.raises(ValueError, match="frames must be"):
        plan.gray_pass(rgb8[..., :1], cs_k, end_k, 255.0, **U8X3)
    with pytest.raises(ValueError, match="frames must be"):
        plan.gray_pass(rgb8, cs_k, end_k, 255.0, frame_dtype="uint8")
    plan.close()


def C_plan(_lib, ctx, hw, levels):
    """A raw single-channel plan handle on ``ctx`` (a context other than the shared one)."""
    import ctypes as C
    arr = (_lib.PyrLevel * len(levels))(*[_lib.PyrLevel(*[int(x) for x in l]) for l in levels])
    handle = C.c_void_p()
    ctx.check(_lib.load().silent_pyramid_plan_create_ex(ctx.handle, hw[0], hw[1], 1, arr, len(levels), 0, C.byref(handle)))
    return handle


# ----------------------------------------------------------------------------- 5. keypoints

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", ["ratio2_3", "reference_crop", "ratio2_3_nostream"])
@pytest.mark.parametrize("selection", [0, 1])
def test_keypoints_equal_those_of_the_float32_frame_entry_point(rt, family, hw, selection):
    """idx, counts, value, peak_value, pyr, cs, end of silent_gray_keypoints_u8x3[_dev] equal silent_gray_keypoints[_dev]'s on the
    frame of values; the host form (PyramidPlan.gray_keypoints) as well."""
    import torch
    from pysilent_amd import _lib
    lib = _lib.load()
    rgb8, v = _batch(hw)
    levels, _ = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    K = 4
    cs_k, end_k = _consts(K)
    n, px = rgb8.shape[0], plan.frame_px
    regions = [(max(eh // 2, 1), max(ew // 2, 1)) for eh, ew in plan.extents]
    reg = (_lib.Extent * len(regions))(*[_lib.Extent(a, b) for a, b in regions])
    s = torch.cuda.current_stream().cuda_stream
    fd = {"rgb8": _t(rgb8).cuda(0), "f32": _t(v).cuda(0)}

    def run(kind):
        f = dict(dtype=torch.float32, device="cuda:0")
        o = {"pyr": torch.full((n * px,), -7.0, **f), "cs": torch.full((n * px,), -7.0, **f), "end": torch.full((n * px * K,), -7.0, **f),
             "value": torch.full((n * px,), -7.0, **f), "peak_value": torch.full((n * px,), -7.0, **f) if selection else None,
             "idx": torch.full((n, px, 4), -1, dtype=torch.int64, device="cuda:0"), "counts": torch.full((n,), -1, dtype=torch.int64, device="cuda:0")}
        ptr = lambda t: None if t is None else t.data_ptr()
        fn = lib.silent_gray_keypoints_u8x3_dev if kind == "rgb8" else lib.silent_gray_keypoints_dev
        fp = _lib.byte_ptr(fd[kind].data_ptr()) if kind == "rgb8" else fd[kind].data_ptr()
        with _Knobs(rt, family):
            plan.ctx.check(fn(plan.ctx.handle, plan.handle, fp, n, cs_k.ctypes.data, end_k.ctypes.data, K, 255.0, ptr(o["pyr"]), ptr(o["cs"]),
                              ptr(o["end"]), 2, selection, 0.1, reg, ptr(o["value"]), ptr(o["peak_value"]), ptr(o["idx"]), px, ptr(o["counts"]), s))
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in o.items() if t is not None}

    want, got = run("f32"), run("rgb8")
    assert (want["counts"] > 0).all() and (want["counts"] <= px).all()
    assert np.array_equal(got["counts"], want["counts"])
    for f in range(n):
        assert np.array_equal(got["idx"][f, :want["counts"][f]], want["idx"][f, :want["counts"][f]]), "frame %d: keypoints differ" % f
    for k in ("pyr", "cs", "end", "value") + (("peak_value",) if selection else ()):
        _same_f32(got[k], want[k], "%s selection=%d %s" % (family, selection, k))
    with _Knobs(rt, family):
        hw_ = plan.gray_keypoints(v, cs_k, end_k, selection=bool(selection))
        hg = plan.gray_keypoints(rgb8, cs_k, end_k, selection=bool(selection), **U8X3)
    for a, b, m in zip(hg[:3], hw_[:3], ("pyramid", "cs", "end")):
        _same_f32(a.data, b.data, "host form %s" % m)
    assert np.array_equal(hg[4], hw_[4]) and np.array_equal(hg[4], want["counts"])
    for f in range(n):
        assert np.array_equal(hg[3][f, :hg[4][f]], want["idx"][f, :want["counts"][f]])
    plan.close()


# ----------------------------------------------------------------------------- 6. pipeline

def _pipe(hw, K, batch, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    kw.setdefault("n_levels", 3)
    return LineEndPipeline(hw, mode="gray", n_orient=K, batch=batch, device=0, **kw)


def _maps(out):
    return {k: out[k].data.clone() for k in ("pyramid", "cs", "end")}


def _same_maps(a, b):
    import torch
    ok = True
    for k in a:
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
            return False
        view = torch.int32 if a[k].dtype == torch.float32 else torch.int16
        ok = ok and torch.equal(a[k].view(view), b[k].view(view))
    return ok


@pytest.mark.parametrize("hw,K", [(pg.FA, 4), (pg.FB, 8)], ids=["150x316-K4", "149x317-K8"])
def test_pipeline_colour_uint8_frames(rt, hw, K):
    """frame_dtype="uint8", frame_channels=3 in step, step_host (pageable ndarray and pinned tensor, consecutive batches with
    different contents, back to back without synchronisation), overlap="force", placement="auto" and storage="float16" gives the maps
    of a float32 pipeline stepped on the frames of values; the ingest slots hold no float32 buffer."""
    import torch
    batch = 2
    rgb_all, v_all = _batch(hw)
    picks = [[0, 1], [2, 3], [3, 0], [1, 2]]
    batches = [np.array(rgb_all[p]) for p in picks]
    ref = _pipe(hw, K, batch)
    want = []
    for p in picks:
        ref.step(_t(v_all[p]).cuda(0))
        want.append(_maps(ref.outputs()))
    assert not _same_maps(want[0], want[1])
    dev = [_t(b).cuda(0) for b in batches]

    u8 = _pipe(hw, K, batch, frame_dtype="uint8")
    base = _pipe(hw, K, batch, **U8X3)
    assert base.frame_dtype == "uint8" and base.frame_channels == 3 and base.frame_shape == (hw[0], hw[1], 3)
    assert base.channels == 1 and base.plan.frame_shape == (hw[0], hw[1], 1) and u8.frame_shape == (hw[0], hw[1], 1)
    assert "3 interleaved channels" in base.launch_summary() and "interleaved" not in u8.launch_summary()
    assert base.dominant_kernel_name() == ref.dominant_kernel_name()
    assert base.algorithmic_bytes_per_frame() == u8.algorithmic_bytes_per_frame() + 2 * hw[0] * hw[1]
    assert base.pyramid_bytes_per_frame() == u8.pyramid_bytes_per_frame() + 2 * hw[0] * hw[1]
    assert base.filter_bytes_per_frame() == u8.filter_bytes_per_frame()
    for i in range(len(batches)):
        base.step(dev[i])
        assert _same_maps(_maps(base.outputs()), want[i]), "step, batch %d" % i
    # the refusals
    with pytest.raises(ValueError, match="uint8"):
        base.step(dev[0].to(torch.float32))
    with pytest.raises(ValueError, match="shape"):
        base.step(dev[0][..., :1].contiguous())
    with pytest.raises(ValueError, match="shape"):
        u8.step(dev[0])
    with pytest.raises(ValueError, match="host frames"):
        base.step_host(dev[0])
    with pytest.raises(ValueError, match="uint8"):
        base.step_host(batches[0].astype(np.float32))
    with pytest.raises(ValueError, match="host frames"):
        base.step_host(batches[0][..., :1])

    # step_host: several consecutive batches with different contents through the ring of two slots, results fetched after each
    # AND only after the whole run (so a slot overwritten too early shows)
    for source in ("pageable", "pinned"):
        host = _pipe(hw, K, batch, **U8X3)
        srcs = [np.array(b) if source == "pageable" else _t(b).pin_memory() for b in batches]
        for i in range(len(batches)):
            host.step_host(srcs[i])
            assert _same_maps(_maps(host.outputs()), want[i]), "step_host (%s), batch %d" % (source, i)
        for i in (1, 2, 3, 0, 2):                       # back to back, no synchronisation in between
            host.step_host(srcs[i])
        assert _same_maps(_maps(host.outputs()), want[2]), "step_host (%s), back to back" % source
        slots = host._ingest[torch.uint8]["slots"]
        assert len(slots) == 2 and all(s["f32"] is None and s["raw"].dtype == torch.uint8 for s in slots)
        assert all(tuple(s["raw"].shape) == (batch, hw[0], hw[1], 3) for s in slots)
        assert list(host._ingest) == [torch.uint8]          # no ring of another dtype: nothing float32 anywhere in the ingest
        assert all((s["pinned"] is None) == (source == "pinned") for s in slots)
        host.close()

    ov = _pipe(hw, K, batch, overlap="force", **U8X3)
    for i in range(len(batches)):
        ov.step(dev[i])
        assert _same_maps(_maps(ov.outputs()), want[i]), "overlap='force', batch %d" % i
    for i in (1, 2, 3, 0, 2, 1):
        ov.step_host(batches[i])
    assert _same_maps(_maps(ov.outputs()), want[1]), "overlap='force' + step_host, back to back"
    assert all(s["f32"] is None for s in ov._ingest[torch.uint8]["slots"])

    tuned = _pipe(hw, K, batch, placement="auto", **U8X3)
    tuned.step(dev[0])
    assert tuned.placement_tuning is not None
    assert _same_maps(_maps(tuned.outputs()), want[0]), "the placement tuner changed the maps"
    # the two tuners on their own synthetic frames (colour uint8 for such a pipeline), with small budgets
    auto = _pipe(hw, K, batch, **U8X3)
    syn = auto._synthetic_frames()
    assert syn.dtype == torch.uint8 and tuple(syn.shape) == (batch, hw[0], hw[1], 3)
    assert auto.tune_overlap(candidates=2, steps=3, budget_s=0.5)["chosen"] in ("one stream", "two streams")
    assert auto.tune_placement(tries=2, steps=3, budget_s=0.3)["tries_ms"]
    auto.step(dev[1])
    assert _same_maps(_maps(auto.outputs()), want[1]), "after tune_overlap / tune_placement"

    ref16 = _pipe(hw, K, batch, storage="float16")
    ref16.step(_t(v_all[picks[1]]).cuda(0))
    h16 = _pipe(hw, K, batch, storage="float16", **U8X3)
    h16.step(dev[1])
    assert h16.cs.dtype == torch.float16 and _same_maps(_maps(h16.outputs()), _maps(ref16.outputs())), "storage='float16'"
    h16.step_host(batches[2])
    ref16.step(_t(v_all[picks[2]]).cuda(0))
    assert _same_maps(_maps(h16.outputs()), _maps(ref16.outputs())), "storage='float16' + step_host"

    # the per-op entry of the pipeline
    base.run_pyramid(dev[3])
    torch.cuda.synchronize()
    assert torch.equal(base.pyr.view(torch.int32), want[3]["pyramid"].view(torch.int32))
    for p in (ref, u8, base, ov, tuned, auto, ref16, h16):
        p.close()


@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
def test_pipeline_colour_uint8_keypoints_with_selection(rt, hw):
    import torch
    batch, K = 2, 4
    rgb_all, v_all = _batch(hw)
    ref = _pipe(hw, K, batch, keypoints=True, selection=True, value_map=True, peak_value_map=True)
    pipe = _pipe(hw, K, batch, keypoints=True, selection=True, value_map=True, peak_value_map=True, **U8X3)
    for i in (0, 2):
        ref.step(_t(v_all[i:i + batch]).cuda(0))
        pipe.step(_t(rgb_all[i:i + batch]).cuda(0))
        want, got = ref.outputs(), pipe.outputs()
        for k in ("pyramid", "cs", "end", "value", "peak_value"):
            assert torch.equal(got[k].data.view(torch.int32), want[k].data.view(torch.int32)), k
        assert np.array_equal(got["keypoint_counts"], want["keypoint_counts"]) and (want["keypoint_counts"] > 0).all()
        for f in range(batch):
            assert np.array_equal(got["keypoints"][f], want["keypoints"][f])
    pipe.step_host(np.array(rgb_all[2:4]))
    got = pipe.outputs()
    assert np.array_equal(got["keypoint_counts"], want["keypoint_counts"])
    assert torch.equal(got["end"].data.view(torch.int32), want["end"].data.view(torch.int32))
    for p in (ref, pipe):
        p.close()


# ----------------------------------------------------------------------------- 7. the C oracle

def test_config1_colour_uint8_frames_against_the_c_oracle(rt):
    """640 x 480, 3 classic levels, K = 4, colour uint8 frames: pyramid, CS and end against the C oracle fed the numpy value frame,
    with the project's tolerance (conftest.assert_close: 1e-5 range-relative + the element-wise rounding bound of tests/err_bound.py)."""
    import c_oracle as co
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, K = (480, 640), 4
    levels = classic_levels(hw, 2.0, 3)
    rgb8 = np.random.default_rng(8801).integers(0, 256, (1, hw[0], hw[1], 3)).astype(np.uint8)
    v = value_of(rgb8)
    cs_k, end_k = _consts(K)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    assert plan.streamable
    pyr, cs, end = plan.gray_pass(rgb8, cs_k, end_k, 255.0, **U8X3)
    for l, lv in enumerate(levels):
        want_pyr = co.zoom_level(v[0], *lv)[None]
        want_cs, want_end = co.gray_line_end_level(want_pyr, cs_k, end_k, 255.0)
        e_pyr = eb.zoom(want_pyr)
        e_cs, e_end = eb.gray_chain(want_pyr, cs_k, end_k, want_cs, e_pyr)
        tag = "config1 colour uint8 %d" % l
        assert_close(pyr.level(l), want_pyr, 1e-5, scale=255.0, what="pyramid " + tag, bound=e_pyr)
        assert_close(cs.level(l), want_cs, 1e-5, scale=255.0, what="cs " + tag, bound=e_cs)
        assert_close(end.level(l), want_end, 1e-5, scale=255.0, what="end " + tag, bound=e_end)
    plan.close()
