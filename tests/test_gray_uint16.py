"""uint16 frames read as they are (silent_*_u16; PyramidPlan.run / gray_pass / gray_keypoints and LineEndPipeline with
frame_dtype="uint16") on the GPU.  uint16 -> float32 is exact (65535 < 2^24) and a uint16 kernel converts the element in a register
at the load, so there is no tolerance: the oracle of everything but the last test is the float32-frame path of the same build on
frames.astype(float32), compared bit for bit -- every element, every level, every frame.  The last test ties the new path to the C
oracle directly.

Frames: the geometry of tests/test_gray_uint8.py -- the 150 x 316 and 149 x 317 frames of tests/plan_geometry.py, batch 4 (two
56-column wave tiles, two tile rows, two region blocks; W % 4 = 0 and 1; the odd 149 x 317 frame stride puts frames 1 and 3 off
8-byte alignment).  Three seeded uint16 noise frames over 0 .. 65535 and one structured frame; a second batch capped at 4095 (12-bit
data, clip_hi = 4095) keeps every map element below 65504, so its float16 maps are finite; a test of its own shows the
overflow-to-inf rule of float16 storage on a saturated block."""
import numpy as np
import pytest

import err_bound as eb
import plan_geometry as pg
from conftest import assert_close, structured_frame
from test_gray_uint8 import FAMILIES, _Knobs, _consts, _levels, _maps, _pipe, _same_f16, _same_f32, _same_maps, _t

pytestmark = pytest.mark.gpu

FRAMES_HW = (pg.FA, pg.FB)
KS = (3, 4, 8)
FULL, TWELVE = 65535.0, 4095.0


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


_BATCH = {}


def _batch(hw, top=65535):
    """(uint16 frames [4, H, W, 1] over 0 .. top, the same widened to float32): computed once, never modified."""
    key = (hw, top)
    if key not in _BATCH:
        noise = [np.random.default_rng(9900 + 13 * hw[1] + i + top).integers(0, top + 1, (hw[0], hw[1], 1)).astype(np.uint16) for i in range(3)]
        noise[0][0, 0, 0], noise[0][0, 1, 0] = 0, top                  # both ends of the range, whatever the draw
        lines = np.clip(structured_frame(31, hw[0], hw[1], 1) * (top / 255.0), 0, top).astype(np.uint16)
        u16 = np.stack(noise + [lines])
        assert u16.dtype == np.uint16 and u16.dtype.isnative and (u16 == 0).any() and (u16 == top).any() and u16.max() == top
        if top == 65535:
            assert (u16 >= 32768).any()                                 # a signed 16-bit load would make these negative
            assert (u16 > 255).any()                                    # a byte load would truncate these
            assert ((u16 & 0xff) != (u16 >> 8)).any()                   # a byte-swapped load would change these
        f32 = u16.astype(np.float32)
        assert np.array_equal(f32.astype(np.int64), u16.astype(np.int64))      # (the widening is exact)
        for a in (u16, f32):
            a.setflags(write=False)
        _BATCH[key] = (u16, f32)
    return _BATCH[key]


def _check_plan(rt, plan, hw, K, knobs, tag):
    """gray_pass (float32 and float16 maps) and run (stream kernel, and unit + region kernels) on uint16 frames against the same calls
    on the widened frames; the 12-bit batch through gray_pass with both storages.  Returns (elements compared, float16 infinities)."""
    from pysilent_amd import _lib
    cs_k, end_k = _consts(K)
    u16, f32 = _batch(hw)
    n = infs = 0
    with knobs:
        want = plan.gray_pass(f32, cs_k, end_k, FULL)
        got = plan.gray_pass(u16, cs_k, end_k, FULL, frame_dtype="uint16")
        want16 = plan.gray_pass(f32, cs_k, end_k, FULL, storage="float16")
        got16 = plan.gray_pass(u16, cs_k, end_k, FULL, storage="float16", frame_dtype="uint16")
    for g, w, m in zip(got, want, ("pyramid", "cs", "end")):
        _same_f32(g.data, w.data, "%s K=%d gray_pass %s" % (tag, K, m))
        n += g.data.size
    _same_f32(got16[0].data, want16[0].data, "%s K=%d float16-map pass: pyramid" % (tag, K))
    for g, w, m in zip(got16[1:], want16[1:], ("cs", "end")):
        _same_f16(g.data, w.data, "%s K=%d float16 %s" % (tag, K, m))
        assert not (np.asarray(g.data) == -np.inf).any()
        infs += int(np.isinf(np.asarray(g.data)).sum())
        n += g.data.size
    for knob in (0, 1):      # pyramid_stream_kernel where the plan streams / pyramid_unit_kernel + pyramid_region_kernel
        with rt.tuning(_lib.TUNE_PYRAMID, knob):
            w = plan.run(f32)
            g = plan.run(u16, frame_dtype="uint16")
        _same_f32(g.data, w.data, "%s run(), PYRAMID knob %d" % (tag, knob))
        _same_f32(g.data, want[0].data, "%s run() vs the gray pass's pyramid, PYRAMID knob %d" % (tag, knob))
        n += g.data.size
    # 12-bit data, clip_hi = 4095: the same identities, and float16 maps without an infinity
    u12, f12 = _batch(hw, 4095)
    with knobs:
        want = plan.gray_pass(f12, cs_k, end_k, TWELVE)
        got = plan.gray_pass(u12, cs_k, end_k, TWELVE, frame_dtype="uint16")
        want16 = plan.gray_pass(f12, cs_k, end_k, TWELVE, storage="float16")
        got16 = plan.gray_pass(u12, cs_k, end_k, TWELVE, storage="float16", frame_dtype="uint16")
    for g, w, m in zip(got, want, ("pyramid", "cs", "end")):
        _same_f32(g.data, w.data, "%s K=%d 12-bit gray_pass %s" % (tag, K, m))
        n += g.data.size
    for g, w, m in zip(got16[1:], want16[1:], ("cs", "end")):
        _same_f16(g.data, w.data, "%s K=%d 12-bit float16 %s" % (tag, K, m))
        assert np.isfinite(np.asarray(g.data)).all(), "%s K=%d 12-bit float16 %s holds an infinity" % (tag, K, m)
        n += g.data.size
    return n, infs


# ----------------------------------------------------------------------------- 1. kernel families

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", FAMILIES)
def test_kernel_families_bit_identical_to_the_float32_frame_path(rt, family, hw):
    levels, streamable = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    assert plan.streamable == streamable, (family, hw)
    n = infs = 0
    for K in KS:
        a, b = _check_plan(rt, plan, hw, K, _Knobs(rt, family), "%s %dx%d" % (family, hw[0], hw[1]))
        n, infs = n + a, infs + b
    print("%s %dx%d: %d elements bit-identical, %d float16 elements +inf with full-range data" % (family, hw[0], hw[1], n, infs))
    plan.close()


def test_float16_maps_overflow_to_inf_exactly_where_the_float32_frame_path_does(rt):
    """float16 storage keeps its rule -- the float32 result rounded to nearest even, overflow to +inf -- with 16-bit data: a block of
    65535 under a CS kernel and an end bank that pass the centre pixel through gives responses of about 65535 > 65504 inside the
    block, stored as +inf by the uint16 path and by silent_gray_pass_h on the widened frame alike; the float32 maps stay finite."""
    hw, K = pg.FA, 4
    u16 = np.array(_batch(hw)[0])
    u16[:, 40:90, 100:200] = 65535
    f32 = u16.astype(np.float32)
    cs_k = np.zeros((3, 3, 1, 1), np.float32)
    cs_k[1, 1] = 1.0
    end_k = np.zeros((3, 3, 1, K), np.float32)
    end_k[1, 1] = 1.0
    plan = rt.PyramidPlan(hw[0], hw[1], 1, _levels("ratio2_3", hw)[0], 0)
    want = plan.gray_pass(f32, cs_k, end_k, FULL, storage="float16")
    got = plan.gray_pass(u16, cs_k, end_k, FULL, storage="float16", frame_dtype="uint16")
    wide = plan.gray_pass(u16, cs_k, end_k, FULL, frame_dtype="uint16")
    for g, w, f, m in zip(got[1:], want[1:], wide[1:], ("cs", "end")):
        _same_f16(g.data, w.data, "float16 %s" % m)
        g16, f_ = np.asarray(g.data), np.asarray(f.data)
        assert np.isposinf(g16).any() and not np.isneginf(g16).any(), m
        assert np.isfinite(f_).all() and np.array_equal(np.isposinf(g16), f_ >= 65520.0), m      # 65520: the first float32 that rounds to inf
    plan.close()


# ----------------------------------------------------------------------------- 2. the base address

@pytest.mark.parametrize("family", ["ratio2_3", "ratio2_3_nostream", "reference_crop"])
def test_base_pointer_off_the_8_byte_grid(rt, family):
    """The uint16 frames pointer is 2-byte aligned, no more: the same 316-wide batch at byte offsets 2, 4 and 6 of a larger device
    buffer gives the outputs of offset 0 (the region kernel's 8-byte group loads are legal at offset 0 only; the others take its
    one-element path)."""
    import torch
    from pysilent_amd import _lib
    hw = pg.FA
    u16, f32 = _batch(hw)
    levels, _ = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    cs_k, end_k = _consts(4)
    with _Knobs(rt, family):
        want = plan.gray_pass(f32, cs_k, end_k, FULL)
    for off in (0, 1, 2, 3):
        host = np.full(u16.size + 32, 0xA5A5, np.uint16)          # (placed on the host, uploaded whole: one plain copy)
        host[off:off + u16.size] = u16.reshape(-1)
        big = _t(host).cuda(0)
        assert big.data_ptr() % 8 == 0
        frames = big[off:off + u16.size].view(u16.shape)
        assert frames.is_contiguous() and frames.data_ptr() % 8 == 2 * off
        with _Knobs(rt, family):
            got = plan.gray_pass(frames, cs_k, end_k, FULL, frame_dtype="uint16")
            runs = []
            for knob in (0, 1):
                with rt.tuning(_lib.TUNE_PYRAMID, knob):
                    runs.append(plan.run(frames, frame_dtype="uint16").data.cpu().numpy())
        torch.cuda.synchronize()
        for g, w, m in zip(got, want, ("pyramid", "cs", "end")):
            _same_f32(g.data.cpu().numpy(), w.data, "%s byte offset %d %s" % (family, 2 * off, m))
        for knob in (0, 1):
            _same_f32(runs[knob], want[0].data, "%s byte offset %d run(), PYRAMID knob %d" % (family, 2 * off, knob))
    plan.close()


# ----------------------------------------------------------------------------- 3. the C ABI: host forms, _dev forms, parts, float16 maps

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", ["ratio2_3", "reference_crop"])
def test_c_abi_host_forms_dev_forms_parts_and_float16_maps(rt, family, hw):
    """silent_gray_pass_u16 / silent_pyramid_u16 on a uint16 ndarray against their _dev forms on a device copy (parts = 3, and parts = 1
    then 2 on poisoned buffers), maps_f16 = 0 against silent_gray_pass and maps_f16 = 1 against the patterns silent_gray_pass_h stores
    for the widened frames; the refusals that need a device to reach."""
    import torch
    from pysilent_amd import _lib
    lib = _lib.load()
    u16, f32 = _batch(hw)
    levels, _ = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    K = 4
    cs_k, end_k = _consts(K)
    n, px = u16.shape[0], plan.frame_px
    h, c = plan.ctx.handle, plan.ctx.check
    want = plan.gray_pass(f32, cs_k, end_k, FULL)
    want16 = plan.gray_pass(f32, cs_k, end_k, FULL, storage="float16")
    frames_h = np.ascontiguousarray(u16)
    frames_d = _t(frames_h).cuda(0)
    s = torch.cuda.current_stream().cuda_stream
    fh, fd = _lib.short_ptr(frames_h.ctypes.data), _lib.short_ptr(frames_d.data_ptr())

    for f16 in (0, 1):
        dt, tdt = (np.float16, torch.float16) if f16 else (np.float32, torch.float32)
        same = _same_f16 if f16 else _same_f32
        ref = want16 if f16 else want
        pyr, cs, end = np.full(n * px, -7.0, np.float32), np.full(n * px, 3.0, dt), np.full(n * px * K, 3.0, dt)
        c(lib.silent_gray_pass_u16(h, plan.handle, fh, n, cs_k.ctypes.data, end_k.ctypes.data, K, FULL, pyr.ctypes.data, cs.ctypes.data,
                                   end.ctypes.data, f16))
        _same_f32(pyr, ref[0].data, "host form pyramid (maps_f16 = %d)" % f16)
        same(cs, ref[1].data, "host form cs (maps_f16 = %d)" % f16)
        same(end, ref[2].data, "host form end (maps_f16 = %d)" % f16)

        def run(parts_seq):
            p = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
            cm = torch.full((n * px,), 3.0, dtype=tdt, device="cuda:0")
            em = torch.full((n * px * K,), 3.0, dtype=tdt, device="cuda:0")
            for parts in parts_seq:
                c(lib.silent_gray_pass_u16_dev(h, plan.handle, fd, n, cs_k.ctypes.data, end_k.ctypes.data, K, FULL, p.data_ptr(),
                                               cm.data_ptr(), em.data_ptr(), f16, parts, s))
            torch.cuda.synchronize()
            return p.cpu().numpy(), cm.cpu().numpy(), em.cpu().numpy()

        whole, halves = run([3]), run([1, 2])
        _same_f32(whole[0], pyr, "_dev form pyramid")
        _same_f32(halves[0], pyr, "parts 1 + 2 pyramid")
        for a, b, r, m in zip(whole[1:], halves[1:], (cs, end), ("cs", "end")):
            same(a, r, "_dev form %s differs from the host form (maps_f16 = %d)" % (m, f16))
            same(b, r, "parts 1 + 2 %s differ from parts = 3 (maps_f16 = %d)" % (m, f16))
    ph = np.full(n * px, -7.0, np.float32)
    c(lib.silent_pyramid_u16(h, plan.handle, fh, n, ph.ctypes.data))
    pd = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
    c(lib.silent_pyramid_u16_dev(h, plan.handle, fd, n, pd.data_ptr(), s))
    torch.cuda.synchronize()
    _same_f32(ph, want[0].data, "silent_pyramid_u16")
    _same_f32(pd.cpu().numpy(), ph, "silent_pyramid_u16_dev")
    # refused before a launch: an odd address, a float64 plan, a 3-channel plan -- every message names its function and "uint16 frames"
    assert lib.silent_pyramid_u16_dev(h, plan.handle, _lib.short_ptr(frames_d.data_ptr() + 1), n, pd.data_ptr(), s) == _lib.SILENT_E_INVALID
    assert "silent_pyramid_u16: uint16 frames" in _lib.last_error(h)
    p64 = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0, accumulation="float64")
    p3 = rt.PyramidPlan(hw[0], hw[1], 3, levels, 0)
    for bad in (p64, p3):
        assert lib.silent_pyramid_u16(h, bad.handle, fh, n, ph.ctypes.data) == _lib.SILENT_E_UNSUPPORTED
        assert "silent_pyramid_u16: uint16 frames" in _lib.last_error(h)
        assert lib.silent_gray_pass_u16(h, bad.handle, fh, n, cs_k.ctypes.data, end_k.ctypes.data, K, FULL, ph.ctypes.data, None, None,
                                        0) == _lib.SILENT_E_UNSUPPORTED
        assert "silent_gray_pass_u16: uint16 frames" in _lib.last_error(h)
        bad.close()
    with pytest.raises(ValueError, match="frame_dtype"):
        rt.PyramidPlan(hw[0], hw[1], 1, levels, 0, accumulation="float64").run(u16, frame_dtype="uint16")
    for wrong in (f32, u16.astype(np.int16), u16.astype(np.uint8), u16.astype(">u2")):
        with pytest.raises(ValueError, match="uint16"):
            plan.gray_pass(wrong, cs_k, end_k, FULL, frame_dtype="uint16")
    plan.close()


# ----------------------------------------------------------------------------- 4. keypoints

@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("family", ["ratio2_3", "reference_crop", "ratio2_3_nostream"])
@pytest.mark.parametrize("selection", [0, 1])
def test_keypoints_equal_those_of_the_float32_frame_entry_point(rt, family, hw, selection):
    """idx, counts, value, peak_value, pyr, cs, end of silent_gray_keypoints_u16[_dev] equal silent_gray_keypoints[_dev]'s on the
    widened frames; the host form (PyramidPlan.gray_keypoints) as well."""
    import torch
    from pysilent_amd import _lib
    lib = _lib.load()
    u16, f32 = _batch(hw)
    levels, _ = _levels(family, hw)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    K = 4
    cs_k, end_k = _consts(K)
    n, px = u16.shape[0], plan.frame_px
    regions = [(max(eh // 2, 1), max(ew // 2, 1)) for eh, ew in plan.extents]
    reg = (_lib.Extent * len(regions))(*[_lib.Extent(a, b) for a, b in regions])
    s = torch.cuda.current_stream().cuda_stream
    fd = {"u16": _t(u16).cuda(0), "f32": _t(f32).cuda(0)}

    def run(kind):
        f = dict(dtype=torch.float32, device="cuda:0")
        o = {"pyr": torch.full((n * px,), -7.0, **f), "cs": torch.full((n * px,), -7.0, **f), "end": torch.full((n * px * K,), -7.0, **f),
             "value": torch.full((n * px,), -7.0, **f), "peak_value": torch.full((n * px,), -7.0, **f) if selection else None,
             "idx": torch.full((n, px, 4), -1, dtype=torch.int64, device="cuda:0"), "counts": torch.full((n,), -1, dtype=torch.int64, device="cuda:0")}
        ptr = lambda t: None if t is None else t.data_ptr()
        fn = lib.silent_gray_keypoints_u16_dev if kind == "u16" else lib.silent_gray_keypoints_dev
        fp = _lib.short_ptr(fd[kind].data_ptr()) if kind == "u16" else fd[kind].data_ptr()
        with _Knobs(rt, family):
            plan.ctx.check(fn(plan.ctx.handle, plan.handle, fp, n, cs_k.ctypes.data, end_k.ctypes.data, K, FULL, ptr(o["pyr"]), ptr(o["cs"]),
                              ptr(o["end"]), 2, selection, 0.1, reg, ptr(o["value"]), ptr(o["peak_value"]), ptr(o["idx"]), px, ptr(o["counts"]), s))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items() if v is not None}

    want, got = run("f32"), run("u16")
    assert (want["counts"] > 0).all() and (want["counts"] <= px).all()
    assert np.array_equal(got["counts"], want["counts"])
    for f in range(n):
        assert np.array_equal(got["idx"][f, :want["counts"][f]], want["idx"][f, :want["counts"][f]]), "frame %d: keypoints differ" % f
    for k in ("pyr", "cs", "end", "value") + (("peak_value",) if selection else ()):
        _same_f32(got[k], want[k], "%s selection=%d %s" % (family, selection, k))
    with _Knobs(rt, family):
        hw_ = plan.gray_keypoints(f32, cs_k, end_k, FULL, selection=bool(selection))
        hg = plan.gray_keypoints(u16, cs_k, end_k, FULL, selection=bool(selection), frame_dtype="uint16")
    for a, b, m in zip(hg[:3], hw_[:3], ("pyramid", "cs", "end")):
        _same_f32(a.data, b.data, "host form %s" % m)
    assert np.array_equal(hg[4], hw_[4]) and np.array_equal(hg[4], want["counts"])
    for f in range(n):
        assert np.array_equal(hg[3][f, :hg[4][f]], want["idx"][f, :want["counts"][f]])
    plan.close()


# ----------------------------------------------------------------------------- 5. pipeline

@pytest.mark.parametrize("hw,K", [(pg.FA, 4), (pg.FB, 8)], ids=["150x316-K4", "149x317-K8"])
def test_pipeline_uint16_frames(rt, hw, K):
    """frame_dtype="uint16" in step, step_host (pageable ndarray and pinned tensor, consecutive batches with different contents),
    overlap="force" and storage="float16" gives the maps of a float32 pipeline stepped on the widened frames."""
    import torch
    batch = 2
    u16_all, _ = _batch(hw)
    batches = [np.array(u16_all[i:i + batch]) for i in (0, 2)] + [np.array(u16_all[[3, 0]]), np.array(u16_all[[1, 2]])]
    ref = _pipe(hw, K, batch, clip_hi=FULL)
    want = []
    for b in batches:
        ref.step(_t(b.astype(np.float32)).cuda(0))
        want.append(_maps(ref.outputs()))
    assert not _same_maps(want[0], want[1])
    dev = [_t(b).cuda(0) for b in batches]

    base = _pipe(hw, K, batch, frame_dtype="uint16", clip_hi=FULL)
    assert base.frame_dtype == "uint16" and "uint16 frames" in base.launch_summary() and "uint16" not in ref.launch_summary()
    assert base.dominant_kernel_name() == ref.dominant_kernel_name()
    assert base.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 2 * hw[0] * hw[1]
    assert base.pyramid_bytes_per_frame() == ref.pyramid_bytes_per_frame() - 2 * hw[0] * hw[1]
    assert base._synthetic_frames().dtype == torch.uint16
    for i in range(len(batches)):
        base.step(dev[i])
        assert _same_maps(_maps(base.outputs()), want[i]), "step, batch %d" % i
    with pytest.raises(ValueError, match="uint16"):
        base.step(dev[0].to(torch.float32))
    with pytest.raises(ValueError, match="float32"):
        ref.step(dev[0])
    with pytest.raises(ValueError, match="host frames"):
        base.step_host(dev[0])
    for wrong in (np.float32, np.uint8, np.int16):
        with pytest.raises(ValueError, match="uint16"):
            base.step_host(batches[0].astype(wrong))

    # step_host: consecutive batches with different contents through the ring of two slots, results fetched after each AND only
    # after a back-to-back run (so a slot overwritten too early shows)
    for source in ("pageable", "pinned"):
        host = _pipe(hw, K, batch, frame_dtype="uint16", clip_hi=FULL)
        srcs = [np.array(b) if source == "pageable" else _t(b).pin_memory() for b in batches]
        for i in range(len(batches)):
            host.step_host(srcs[i])
            assert _same_maps(_maps(host.outputs()), want[i]), "step_host (%s), batch %d" % (source, i)
        for i in (1, 2, 3, 0, 2):                       # back to back, no synchronisation in between
            host.step_host(srcs[i])
        assert _same_maps(_maps(host.outputs()), want[2]), "step_host (%s), back to back" % source
        slots = host._ingest[torch.uint16]["slots"]     # no cast launch, no float32 slot buffer: 2 B/px on the device
        assert len(slots) == 2 and all(s["f32"] is None and s["raw"].dtype == torch.uint16 for s in slots)
        assert all((s["pinned"] is None) == (source == "pinned") for s in slots)
        host.close()

    ov = _pipe(hw, K, batch, frame_dtype="uint16", overlap="force", clip_hi=FULL)
    for i in range(len(batches)):
        ov.step(dev[i])
        assert _same_maps(_maps(ov.outputs()), want[i]), "overlap='force', batch %d" % i
    for i in (1, 2, 3, 0, 2, 1):
        ov.step_host(batches[i])
    assert _same_maps(_maps(ov.outputs()), want[1]), "overlap='force' + step_host, back to back"

    u12 = np.array(_batch(hw, 4095)[0][:batch])
    ref16 = _pipe(hw, K, batch, storage="float16", clip_hi=TWELVE)
    ref16.step(_t(u12.astype(np.float32)).cuda(0))
    h16 = _pipe(hw, K, batch, storage="float16", frame_dtype="uint16", clip_hi=TWELVE)
    h16.step(_t(u12).cuda(0))
    assert h16.cs.dtype == torch.float16 and _same_maps(_maps(h16.outputs()), _maps(ref16.outputs())), "storage='float16'"
    assert torch.isfinite(h16.end).all() and torch.isfinite(h16.cs).all()

    base.run_pyramid(dev[3])
    torch.cuda.synchronize()
    assert torch.equal(base.pyr.view(torch.int32), want[3]["pyramid"].view(torch.int32))
    for p in (ref, base, ov, ref16, h16):
        p.close()


@pytest.mark.parametrize("hw", FRAMES_HW, ids=lambda hw: "%dx%d" % hw)
def test_pipeline_uint16_keypoints_with_selection(rt, hw):
    import torch
    batch, K = 2, 4
    u16_all, _ = _batch(hw)
    kw = dict(keypoints=True, selection=True, value_map=True, peak_value_map=True, clip_hi=FULL)
    ref = _pipe(hw, K, batch, **kw)
    pipe = _pipe(hw, K, batch, frame_dtype="uint16", **kw)
    for i in (0, 2):
        b = np.array(u16_all[i:i + batch])
        ref.step(_t(b.astype(np.float32)).cuda(0))
        pipe.step(_t(b).cuda(0))
        want, got = ref.outputs(), pipe.outputs()
        for k in ("pyramid", "cs", "end", "value", "peak_value"):
            assert torch.equal(got[k].data.view(torch.int32), want[k].data.view(torch.int32)), k
        assert np.array_equal(got["keypoint_counts"], want["keypoint_counts"]) and (want["keypoint_counts"] > 0).all()
        for f in range(batch):
            assert np.array_equal(got["keypoints"][f], want["keypoints"][f])
    pipe.step_host(np.array(u16_all[2:4]))
    got = pipe.outputs()
    assert np.array_equal(got["keypoint_counts"], want["keypoint_counts"])
    assert torch.equal(got["end"].data.view(torch.int32), want["end"].data.view(torch.int32))
    for p in (ref, pipe):
        p.close()


# ----------------------------------------------------------------------------- 6. the C oracle

def test_config1_p010_frames_against_the_c_oracle(rt):
    """640 x 480, 3 classic levels, K = 4, uint16 frames as a P010 decoder delivers luma -- 10-bit noise in the HIGH bits (v << 6),
    clip_hi = 1023 * 64 --: pyramid, CS and end against the C oracle on the widened frame with the project's tolerance
    (conftest.assert_close: 1e-5 range-relative + the element-wise rounding bound of tests/err_bound.py), scale = 1023 * 64.  Every
    term of that tolerance is a multiple of the data's scale, and so is every float32 rounding error of the pass (it is homogeneous of
    degree one up to clip_hi and a factor of 64 is exact), so the oracle's own float32-against-float64 differences sit where they sit
    for 0 .. 1023 data, relative to the range -- the same place as in the uint8 suite's test on 0 .. 255."""
    import c_oracle as co
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw, K = (480, 640), 4
    top = 1023.0 * 64
    levels = classic_levels(hw, 2.0, 3)
    u16 = (np.random.default_rng(8816).integers(0, 1024, (1, hw[0], hw[1], 1)) << 6).astype(np.uint16)
    assert u16.max() == 1023 * 64 and (u16 >= 32768).any()
    f32 = u16.astype(np.float32)
    cs_k, end_k = _consts(K)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    assert plan.streamable
    pyr, cs, end = plan.gray_pass(u16, cs_k, end_k, top, frame_dtype="uint16")
    for l, lv in enumerate(levels):
        want_pyr = co.zoom_level(f32[0], *lv)[None]
        want_cs, want_end = co.gray_line_end_level(want_pyr, cs_k, end_k, top)
        e_pyr = eb.zoom(want_pyr)
        e_cs, e_end = eb.gray_chain(want_pyr, cs_k, end_k, want_cs, e_pyr)
        tag = "config1 uint16 %d" % l
        assert_close(pyr.level(l), want_pyr, 1e-5, scale=top, what="pyramid " + tag, bound=e_pyr)
        assert_close(cs.level(l), want_cs, 1e-5, scale=top, what="cs " + tag, bound=e_cs)
        assert_close(end.level(l), want_end, 1e-5, scale=top, what="end " + tag, bound=e_end)
    plan.close()
