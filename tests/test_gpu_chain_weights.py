"""Every kernel form of the two fused chains on CLASS-GENERIC weights (tests/chain_weights.py) instead of the reference's own very
symmetric constants: against the oracle with the project's tolerance (1e-5 range-relative + the element-wise rounding bound of
tests/err_bound.py), between two float32 evaluation orders within 2e-6 of the range, everything else bit for bit.
tests/test_chain_weights.py shows on the CPU that these assertions are attainable in float32 and that no dy <-> dx, mirror,
i <-> o, channel-0-profile or blur-axis mix-up in a kernel could pass them."""
import math

import numpy as np
import pytest

import chain_weights as cw
import err_bound as eb
import silent_oracle as so
from conftest import assert_close, assert_regulated_close, noise_frame, structured_frame
from pysilent_amd._lib import TUNE_GRAY, TUNE_RGB

pytestmark = pytest.mark.gpu

RTOL = 1e-5
RGB = sorted(cw.RGB_BUILDERS)
FUSED = sorted(cw.RGB_VARIANTS)            # the classes of the single-launch kernels (the non-uniform blur takes the staged path)


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), "%s: NaN pattern differs" % what
    np.testing.assert_array_equal(np.nan_to_num(a, nan=7.0).view(np.int32), np.nan_to_num(b, nan=7.0).view(np.int32), err_msg=what)


def _same_maps(a, b, what):
    for name in ("orient", "line_end", "value"):
        x, y = a[name], b[name]
        _same_bits(getattr(x, "data", x), getattr(y, "data", y), "%s %s" % (name, what))


def _f16_bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float16
    b = a.view(np.uint16).copy()
    b[np.isnan(a)] = 0x7e00
    return b


# ----------------------------------------------------------------------------- RGB chain

def _against_oracle(rt, x, ks, policy, params, tag, isolate=True):
    rv, root, clip, pad = params
    got = rt.rgb_line_end(x, ks, regulation_value=rv, regulation_root=root, flat_policy=policy, clip_hi=clip, pad=pad)
    want = so.rgb_line_end_chain(x, ks, policy, root, rv, clip, pad)
    bound = eb.rgb_chain(x, ks, want, policy, root, rv, pad)
    cw.assert_rgb_chain_close(got, want, bound, clip, tag)
    if isolate:     # each later stage against the oracle continued from the GPU's own map
        g_orient = np.ascontiguousarray(got["orient"])
        p = [[0, 0], [pad, pad], [pad, pad], [0, 0]]
        le = so.pad_inwards(so.conv2d_same(g_orient, ks["end"], relu=True, clip_hi=clip), p)
        assert_close(got["line_end"], le, RTOL, what="line_end|gpu-orient " + tag, bound=eb.pad(eb.conv(g_orient, ks["end"]), pad))
        np.testing.assert_array_equal(got["value"], so.value_from_color(np.ascontiguousarray(got["line_end"])))
    return got, want


@pytest.mark.parametrize("policy", ["zero", "ieee"])
@pytest.mark.parametrize("name", RGB)
def test_rgb_chain_against_the_oracle(rt, name, policy):
    """Noise frames, a line drawing (exact zeros: the 0 * inf pattern under 'ieee') and the frames on which the regulator is active,
    at the wave / tile edges of the chain kernels."""
    ks = cw.rgb_weights(name)
    tag = "%s %s" % (name, policy)
    for shape in cw.RGB_SHAPES:
        x = cw.rgb_frames(shape)
        got, want = _against_oracle(rt, x, ks, policy, cw.PARAM_SETS[0], tag)
        if policy == "ieee" and shape[0] > 1:
            assert np.isnan(want["orient"][1]).any() and not np.isnan(want["orient"][0]).any()
    _against_oracle(rt, cw.dim_frames(), ks, policy, cw.PARAM_SETS[0], tag + " dim")


@pytest.mark.parametrize("policy", ["zero", "ieee"])
@pytest.mark.parametrize("name", RGB)
def test_rgb_chain_nondefault_parameters(rt, name, policy):
    """regulation_value != 1, another root, clip_hi != 255, pad 1 / 0, and pad = 3 on a level the mask empties."""
    ks = cw.rgb_weights(name)
    x = cw.param_frames()
    for params in cw.PARAM_SETS:
        _against_oracle(rt, x, ks, policy, params, "%s %s rv %g" % (name, policy, params[0]))
    small = noise_frame(77, 6, 40, 3)[None]                 # 6 rows <= 2 * pad: nothing is left of line_end / value
    got, want = _against_oracle(rt, small, ks, policy, (0.7, 0.25, 100.0, 3), "%s %s pad 3" % (name, policy))
    assert not want["padded"].any() and not np.asarray(got["line_end"]).any() and not np.asarray(got["value"]).any()
    packed = rt.PackedPyramid.from_levels([noise_frame(78, 23, 40, 3)[None], small])
    both = rt.rgb_line_end(packed, ks, flat_policy=policy, pad=3)
    assert both["line_end"].level(0).any() and not both["line_end"].level(1).any()


@pytest.mark.parametrize("name", ["symmetric", "dense", "basic_blur"])
def test_rgb_chain_on_plateau_frames_by_the_three_zone_rule(rt, name):
    """Flat coloured blocks, a black region and a flat grey one under 'ieee' (the frames of
    test_rgb_chain_on_plateau_frames_under_ieee_by_the_three_zone_rule): where the summation order decides between NaN and residue
    the deterministic rule of conftest.assert_regulated_close applies."""
    ks = cw.rgb_weights(name)
    rng = np.random.default_rng(21)
    frames = np.floor(rng.random((2, 96, 150, 3)) * 4).astype(np.float32) * 64
    frames = np.repeat(np.repeat(frames[:, ::6, ::6], 6, axis=1), 6, axis=2)[:, :96, :150]
    frames[0, 20:60, 30:90] = 0.0
    frames[1, :, 100:] = 128.0
    got = rt.rgb_line_end(frames, ks, flat_policy="ieee")
    want = so.rgb_line_end_chain(frames, ks, "ieee")
    b = so.conv2d_same(want["stripe"], ks["blur"])
    assert_regulated_close(got["orient"], want["stripe"], b, want["orient"], RTOL, what="plateau orient " + name)
    assert np.isnan(want["orient"]).sum() > 1000
    g_orient = np.ascontiguousarray(got["orient"])
    le = so.pad_inwards(so.conv2d_same(g_orient, ks["end"], relu=True, clip_hi=255.0), [[0, 0], [2, 2], [2, 2], [0, 0]])
    assert_close(got["line_end"], le, RTOL, what="plateau line_end|gpu-orient " + name, bound=eb.pad(eb.conv(g_orient, ks["end"]), 2))
    np.testing.assert_array_equal(got["value"], so.value_from_color(np.ascontiguousarray(got["line_end"])))


def _poisoned(frames):
    frames = frames.copy()
    n, h, w, _ = frames.shape
    if h > 8:
        frames[0, 3:9, : max(1, w // 3)] = 0.0            # a flat region: 0 * inf under 'ieee'
    if h * w > 64:
        rng = np.random.default_rng(h * 1000 + w)
        ys, xs = rng.integers(0, h, 4), rng.integers(0, w, 4)
        for k, v in enumerate((np.nan, -np.nan, np.inf, -np.inf)):
            frames[0, ys[k], xs[k], (k + 1) % 3] = v
    return frames


def test_rgb_knob_ladder_on_the_symmetric_class(rt):
    """SILENT_TUNE_RGB 0 / 64 / 2 / 1 move the symmetric class's weights through the symmetric, two-group, basic and dense
    instantiation: each against the oracle; symmetric vs two-group within 2e-6 of the range with the same NaN / inf footprint; the
    pair kernel vs the one-pixel kernel (bit 4) and 18- vs 90-row tiles (bit 3) bit-identical."""
    ks = cw.rgb_weights("symmetric")
    for shape in cw.RGB_SHAPES:
        clean = cw.rgb_frames(shape)
        want = so.rgb_line_end_chain(clean, ks, "zero")
        bound = eb.rgb_chain(clean, ks, want, "zero")
        outs = {}
        for knob in (0, 64, 2, 1):
            with rt.tuning(TUNE_RGB, knob):
                outs[knob] = rt.rgb_line_end(clean, ks, flat_policy="zero")
            cw.assert_rgb_chain_close(outs[knob], want, bound, 255.0, "symmetric knob %d" % knob)
        for name in ("orient", "line_end", "value"):
            assert_close(outs[0][name], outs[64][name], 2e-6, scale=255.0, what=name + " symmetric vs two-group (generic)", rel_floor=None)
        if shape[1] * shape[2] > 1000:            # really different code paths
            assert not np.array_equal(outs[0]["orient"], outs[64]["orient"]) and not np.array_equal(outs[64]["orient"], outs[1]["orient"])
        bad = _poisoned(clean)
        for policy in ("ieee", "zero"):
            with rt.tuning(TUNE_RGB, 0):
                sym = rt.rgb_line_end(bad, ks, flat_policy=policy)
            with rt.tuning(TUNE_RGB, 8):
                _same_maps(sym, rt.rgb_line_end(bad, ks, flat_policy=policy), "symmetric tall tiles " + policy)
            with rt.tuning(TUNE_RGB, 64):
                two = rt.rgb_line_end(bad, ks, flat_policy=policy)
            for name in ("orient", "line_end", "value"):
                a, b = np.asarray(sym[name]), np.asarray(two[name])
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), (name, policy, shape)
                inf = np.isinf(b)
                np.testing.assert_array_equal(np.signbit(a[inf]), np.signbit(b[inf]))
            for knob in (64, 2, 1):
                for tall in (0, 8):
                    with rt.tuning(TUNE_RGB, knob | tall):
                        pair = rt.rgb_line_end(bad, ks, flat_policy=policy)
                    with rt.tuning(TUNE_RGB, knob | tall | 16):
                        one = rt.rgb_line_end(bad, ks, flat_policy=policy)
                    _same_maps(pair, one, "pair vs one-pixel knob %d %s %s" % (knob | tall, policy, shape))


@pytest.mark.parametrize("name", ["two_group", "basic_blur", "basic_masks", "basic_dense", "dense"])
def test_rgb_pair_kernel_equals_the_one_pixel_kernel_on_the_other_classes(rt, name):
    """The classes that reach the two-group, basic and dense instantiation by DETECTION (knob 0): pair kernel vs one-pixel kernel
    and both tile heights, bit for bit, with NaN / inf pixels and a flat region."""
    ks = cw.rgb_weights(name)
    for shape in cw.RGB_SHAPES:
        bad = _poisoned(cw.rgb_frames(shape))
        for policy in ("ieee", "zero"):
            pair = rt.rgb_line_end(bad, ks, flat_policy=policy)
            for knob in (16, 8, 8 | 16):
                with rt.tuning(TUNE_RGB, knob):
                    _same_maps(pair, rt.rgb_line_end(bad, ks, flat_policy=policy), "%s knob %d %s %s" % (name, knob, policy, shape))


@pytest.mark.parametrize("name", FUSED)
def test_rgb_16_byte_stores_are_bit_identical(rt, name):
    """SILENT_TUNE_RGB bit 7 on a ragged pyramid whose rows start on 16-byte boundaries (widths multiples of 4)."""
    levels = cw.store_levels()
    packed = rt.PackedPyramid.from_levels(levels)
    ks = cw.rgb_weights(name)
    for tall in (0, 8):
        with rt.tuning(TUNE_RGB, tall):
            a = rt.rgb_line_end(packed, ks)
        with rt.tuning(TUNE_RGB, 128 | tall):
            b = rt.rgb_line_end(packed, ks)
        _same_maps(a, b, "%s 16-byte stores, tall %d" % (name, tall))
    for l, lev in enumerate(levels[:2]):        # and the packed launch itself against the oracle
        want = so.rgb_line_end_chain(lev, ks)
        got = {n: a[n].level(l) for n in ("orient", "line_end", "value")}
        cw.assert_rgb_chain_close(got, want, eb.rgb_chain(lev, ks, want), 255.0, "%s packed" % name)


@pytest.mark.parametrize("policy", ["zero", "ieee"])
def test_rgb_staged_path_on_a_packed_pyramid(rt, policy):
    """A blur that differs per (i, o): rgb_chain_launch's staged path through workspace temporaries, two packed levels."""
    ks = cw.rgb_weights("nonuniform_blur")
    levels = cw.staged_levels()
    got = rt.rgb_line_end(rt.PackedPyramid.from_levels(levels), ks, flat_policy=policy)
    for l, lev in enumerate(levels):
        want = so.rgb_line_end_chain(lev, ks, policy)
        g = {n: got[n].level(l) for n in ("orient", "line_end", "value")}
        cw.assert_rgb_chain_close(g, want, eb.rgb_chain(lev, ks, want, policy), 255.0, "staged %s" % policy)


@pytest.mark.parametrize("name", RGB)
def test_rgb_nonfinite_pixels_against_the_oracle(rt, name):
    """NaN / -NaN / +inf / -inf pixels: the reference's dense convolutions form every product, so 0 * inf = NaN reaches every output
    of a channel-diagonal kernel -- the diagonal forms must reproduce that with their poison term, the dense class has no zero
    weight at all.  Same NaN pattern, same infinities, finite values within the tolerance."""
    ks = cw.rgb_weights(name)
    for shape in [(2, 70, 131, 3), (1, 19, 5, 3), (1, 2, 3, 3)]:
        n, h, w, _ = shape
        rng = np.random.default_rng(h * 1000 + w)
        frames = np.stack([noise_frame(250 + i, h, w, 3) for i in range(n)])
        if h > 8:
            frames[0, 3:9, : max(1, w // 3)] = 0.0
        bad = [np.nan, -np.nan, np.inf, -np.inf]
        spots = [(0, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0)] + [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(6)]
        for k, (y, x) in enumerate(spots):
            frames[0, y, x, k % 3] = bad[k % 4]
        if h > 20 and w > 20:
            frames[0, 15, 15, 0], frames[0, 15, 16, 0] = np.inf, -np.inf
            frames[0, 18, 5] = [np.inf, np.nan, -np.inf]
        for policy in ("ieee", "zero"):
            want = so.rgb_line_end_chain(frames, ks, policy)
            got = rt.rgb_line_end(frames, ks, flat_policy=policy)
            for m, ref in (("orient", "orient"), ("line_end", "padded"), ("value", "value")):
                a, b = np.asarray(got[m]), want[ref]
                assert np.array_equal(np.isnan(a), np.isnan(b)), "%s %s %s: NaN pattern differs (%d vs %d)" % (
                    name, m, policy, np.isnan(a).sum(), np.isnan(b).sum())
                inf = np.isinf(b)
                assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), (name, m, policy)
                fin = np.isfinite(b)
                if fin.any():
                    assert_close(np.where(fin, a, 0), np.where(fin, b, 0), RTOL, scale=max(float(np.abs(b[fin]).max()), 1.0),
                                 what="%s %s non-finite pixels (generic)" % (m, policy), rel_floor=None)


@pytest.mark.parametrize("name", RGB)
def test_rgb_keypoints_composite_equals_chain_then_selection(rt, name):
    """silent_rgb_keypoints on each class against silent_rgb_line_end + silent_select_keypoints on the GPU's own maps, bit for bit.
    Only the two-group instantiations accumulate the extrema inside the chain kernel, so the basic and dense classes take the
    reduction pass (level_maxmin_kernel) and the dense tail, and a per-(i, o) blur takes a branch of its own (staged chain through
    the context workspace, then silent_select_keypoints): the sparse tail runs exactly for variants 2 and 3.  All pipelines share one
    context, so each class's step comes right AFTER a step whose sparse tail ran: silent_sparse_tail_stats must describe the last
    call, not that one."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    ks = cw.rgb_weights(name)
    hw = cw.PIPELINE_HW
    frames = cw.pipeline_frames()
    common = dict(mode="rgb", n_levels=4, batch=3, selection=True, max_keypoints_per_frame=1 << 16)
    fused, plain = LineEndPipeline(hw, constants=ks, **common), LineEndPipeline(hw, constants=ks, **common)
    sparse = LineEndPipeline(hw, value_map=False, peak_value_map=False, constants=ks, **common)
    primer = LineEndPipeline(hw, value_map=False, peak_value_map=False, constants=cw.rgb_weights("symmetric"), **common)
    t = torch.from_numpy(frames).cuda()
    fused.step(t)
    plain.run_pyramid(t)
    plain.run_filters()
    plain.run_keypoints()
    primer.step(t)
    assert primer.sparse_tail_stats()["ran"]
    sparse.step(t)
    stats = sparse.sparse_tail_stats()
    torch.cuda.synchronize()
    variant = cw.RGB_VARIANTS[name][0] if name in cw.RGB_VARIANTS else -1          # (-1: the staged path)
    assert stats["ran"] == (variant >= 2), (name, stats)
    if not stats["ran"]:
        assert stats["pairs"] == stats["dense_pairs"] == stats["zero_map_pairs"] == stats["candidates"] == 0, stats
    a, b, c = fused.outputs(), plain.outputs(), sparse.outputs()
    for m in ("orient", "line_end", "value", "peak_value"):
        _same_bits(a[m].data.cpu().numpy(), b[m].data.cpu().numpy(), "%s %s" % (name, m))
    for got in (a, c):
        np.testing.assert_array_equal(got["keypoint_counts"], b["keypoint_counts"])
        for f in range(3):
            np.testing.assert_array_equal(got["keypoints"][f], b["keypoints"][f])
    assert sum(len(k) for k in a["keypoints"]) > 0
    # and the maps the keypoints come from are the oracle's, level 1 of the noise frame
    lev = np.ascontiguousarray(a["pyramid"].level(1)[0:1].cpu().numpy())
    want = so.rgb_line_end_chain(lev, ks)
    g = {m: a[m].level(1)[0:1].cpu().numpy() for m in ("orient", "line_end", "value")}
    cw.assert_rgb_chain_close(g, want, eb.rgb_chain(lev, ks, want), 255.0, "%s pipeline" % name)


# ----------------------------------------------------------------------------- gray chain

def _gray(K):
    return cw.gray_cs(cw.SEED), cw.gray_bank(K, cw.SEED)


@pytest.mark.parametrize("K", [3, 4, 8])
def test_gray_line_end_fused(rt, K):
    cs_k, bank = _gray(K)
    levels = cw.gray_levels(20 + K)
    packed = rt.PackedPyramid.from_levels(levels)
    cs, end = rt.gray_line_end(packed, cs_k, bank)
    cs2 = rt.conv2d_same(packed, cs_k, relu=True)
    end2 = rt.conv2d_same(cs2, bank, relu=True, clip_hi=255.0)
    np.testing.assert_array_equal(cs.data, cs2.data)            # same fma order -> bit-identical
    np.testing.assert_array_equal(end.data, end2.data)
    for l, lev in enumerate(levels):
        want_cs, want_end = so.gray_line_end_pass([lev], cs_k, bank)[0]
        cw.assert_gray_chain_close(cs.level(l), end.level(l), lev, want_cs, want_end, cs_k, bank, "generic K=%d" % K)
        gcs = np.ascontiguousarray(cs.level(l))
        assert_close(end.level(l), so.conv2d_same(gcs, bank, relu=True, clip_hi=255.0), RTOL, what="end|gpu-cs generic K=%d" % K,
                     bound=eb.conv(gcs, bank))


def assert_gray_level_close(got_pyr, got_cs, got_end, want_pyr, want_cs, want_end, cs_kernel, bank, tag):
    """As in tests/test_gpu_parity.py: pyramid level, CS map and line-end maps against the oracle's, range-relative 1e-5 and, element
    by element, the propagated rounding bound."""
    e_pyr = eb.zoom(want_pyr)
    e_cs, e_end = eb.gray_chain(want_pyr, cs_kernel, bank, want_cs, e_pyr)
    assert_close(got_pyr, want_pyr, RTOL, scale=255.0, what="pyramid " + tag, bound=e_pyr)
    assert_close(got_cs, want_cs, RTOL, scale=255.0, what="cs " + tag, bound=e_cs)
    assert_close(got_end, want_end, RTOL, scale=255.0, what="end " + tag, bound=e_end)


def _gray_plans():
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    return [
        ("stream", (270, 480), classic_levels((270, 480), 2.0, 8), 2.0, 8, 4),                 # 7 general levels: stream kernel <K, 7>
        ("dense slots", (216, 384), classic_levels((216, 384), 2 ** .5, 6), 2 ** .5, 6, 3),   # the dense slot layout
        ("region", (100, 260), classic_levels((100, 260), 1.2, 3), 1.2, 3, 8),                 # not stream-eligible
        ("crop", (240, 320), reference_levels((240, 320), (80, 60), math.e ** .5), None, None, 4),
        ("tiny", (4, 9), classic_levels((4, 9), 2.0, 2), 2.0, 2, 4),
        ("tile", (25, 225), classic_levels((25, 225), 2.0, 2), 2.0, 2, 8),
    ]


@pytest.mark.parametrize("plan_id", range(6))
def test_gray_pass_routes(rt, plan_id):
    """One plan per route of silent_gray_pass: bit-identical to plan.run + gray_line_end, the oracle's maps within the tolerance;
    float16 storage = the float32 maps rounded to nearest even, bit for bit; float64 accumulation = the oracle applied to the GPU's
    own pyramid, bit for bit."""
    import c_oracle as co
    tag, hw, levels, scale, n, K = _gray_plans()[plan_id]
    cs_k, bank = _gray(K)
    frames = np.stack([noise_frame(s, hw[0], hw[1], 1) for s in range(2)])
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels)
    if tag in ("stream", "dense slots", "region", "crop"):
        assert plan.streamable == (tag in ("stream", "dense slots"))      # which path silent_gray_pass takes for this plan
    pyr, cs, end = plan.gray_pass(frames, cs_k, bank)
    pyr2 = plan.run(frames)
    cs2, end2 = rt.gray_line_end(pyr2, cs_k, bank)
    for a, b in ((pyr, pyr2), (cs, cs2), (end, end2)):
        np.testing.assert_array_equal(a.data, b.data)
    if scale is not None:
        want = so.classic_pyramid(frames[1], scale, n)
        for l, (wcs, wend) in enumerate(so.gray_line_end_pass(want, cs_k, bank)):
            assert_gray_level_close(pyr.level(l)[1:2], cs.level(l)[1:2], end.level(l)[1:2], want[l], wcs, wend, cs_k, bank, "generic " + tag)
    else:
        want = so.zoom_from_image(frames[1], 1, (80, 60), math.e ** .5)
        h, w = plan.extents[0]
        got = np.stack([pyr.level(l)[1] for l in range(len(levels))]).reshape(want.shape)
        wcs = so.conv2d_same(want, cs_k, relu=True)
        wend = so.conv2d_same(wcs, bank, relu=True, clip_hi=255.0)
        gcs = np.stack([cs.level(l)[1] for l in range(len(levels))]).reshape(wcs.shape)
        gend = np.stack([end.level(l)[1] for l in range(len(levels))]).reshape(wend.shape)
        assert_gray_level_close(got, gcs, gend, want, wcs, wend, cs_k, bank, "generic " + tag)
    # float16 storage
    p16, cs16, end16 = plan.gray_pass(frames, cs_k, bank, storage="float16")
    np.testing.assert_array_equal(p16.data, pyr.data)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(_f16_bits(cs16.data), _f16_bits(np.asarray(cs.data, np.float32).astype(np.float16)))
        np.testing.assert_array_equal(_f16_bits(end16.data), _f16_bits(np.asarray(end.data, np.float32).astype(np.float16)))
    plan.close()
    # float64 accumulation
    plan64 = rt.PyramidPlan(hw[0], hw[1], 1, levels, accumulation="float64")
    p64, cs64, end64 = plan64.gray_pass(frames, cs_k, bank)
    k_cs, k_end = np.ascontiguousarray(cs_k, np.float32), np.ascontiguousarray(bank, np.float32)
    for f in range(2):
        for l, (h, w) in enumerate(plan64.extents):
            lev = np.ascontiguousarray(p64.level(l)[f].reshape(h, w))
            want_cs, want_end = co.gray_line_end_level(lev[None, :, :, None], k_cs, k_end, 255.0)
            _same_bits(cs64.level(l)[f].reshape(h, w), want_cs[0, :, :, 0], "float64 cs %s level %d" % (tag, l))
            _same_bits(end64.level(l)[f].reshape(h, w, K), want_end[0], "float64 end %s level %d" % (tag, l))
    plan64.close()


@pytest.mark.parametrize("K", [3, 4, 8])
@pytest.mark.parametrize("selection", [True, False])
def test_gray_keypoints_equal_the_pass_then_selection(rt, K, selection):
    """silent_gray_keypoints (selection 0 / 1, sparse and -- SILENT_TUNE_GRAY bit 6 -- dense tail) against silent_gray_pass followed by
    the separate selection calls on the GPU's own end map: maps and keypoint rows bit for bit."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    cs_k, bank = _gray(K)
    hw = (130, 210)
    frames = np.stack([noise_frame(11 + K, hw[0], hw[1], 1), structured_frame(12 + K, hw[0], hw[1], 1)])
    plan = rt.PyramidPlan(hw[0], hw[1], 1, classic_levels(hw, 2.0, 3))
    regions = [(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents]
    pyr, cs, end = plan.gray_pass(frames, cs_k, bank)
    color = rt.pad_inwards(end, 2, 2, 2, 2)
    value = rt.value_from_color(color)
    v = rt.value_from_color(rt.nms3x3(rt.top_value_points(color, 0.1, value))) if selection else value
    want_idx, want_counts = rt.max_value_indices_region(v, regions)
    assert want_counts.sum() > 0
    for knob in (0, 64):
        with rt.tuning(TUNE_GRAY, knob):
            p2, cs2, end2, idx, counts = plan.gray_keypoints(frames, cs_k, bank, selection=selection, regions=regions)
        for a, b in ((pyr, p2), (cs, cs2), (end, end2)):
            np.testing.assert_array_equal(a.data, b.data)
        np.testing.assert_array_equal(counts, want_counts)
        for f in range(2):
            np.testing.assert_array_equal(idx[f, :counts[f]], want_idx[f, :want_counts[f]], err_msg="frame %d knob %d" % (f, knob))
    plan.close()
