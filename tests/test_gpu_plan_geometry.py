"""Pyramid plans on level geometry classic_levels() / reference_levels() never produce (tests/plan_geometry.py): sub-window
ladders at every alignment, unit levels anywhere and any number, anisotropic and upsampled levels, canvases around their zoom,
off-centre / overlapping / disjoint crops, degenerate axes.  Against the C oracle per level with the project's tolerance (1e-5
range-relative + the element-wise rounding bound of tests/err_bound.py); everything the header calls "same results" bit for bit.
tests/test_plan_geometry.py shows on the CPU that the assertion is attainable in float32, that no crop-origin, mirror, per-axis,
order, offset or clipping mistake could pass it, and which kernels each case reaches."""
import ctypes as C

import numpy as np
import pytest

import chain_weights as cw
import plan_geometry as pg
from pysilent_amd._lib import TUNE_GRAY, TUNE_PYRAMID

pytestmark = pytest.mark.gpu

NAMES = sorted(pg.CASES)
KS = (3, 4, 8)


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


_CACHE = {}


def _case(name, channels):
    """(frame_hw, levels, frames [3, H, W, C], the oracle's levels of the last frame): computed once, never modified."""
    key = (name, channels)
    if key not in _CACHE:
        case = pg.CASES[name]
        frames = pg.frames_of(case["frame"], channels, 3, seed=NAMES.index(name))
        want = pg.oracle_pyramid(frames[-1], case["levels"])
        for a in [frames] + want:
            a.setflags(write=False)
        _CACHE[key] = (case["frame"], case["levels"], frames, want)
    return _CACHE[key]


def _route(name, channels):
    streamable, walk = pg.ROUTES[name][0 if channels == 1 else 1]
    return "+".join(sorted(pg.route_tags(pg.CASES[name]["levels"], channels, streamable, walk)))


def _bits(a):
    """int32 patterns with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _levels_of(packed, f, levels, channels):
    return pg.split(np.asarray(packed.data).reshape(packed.n_frames, -1)[f], levels, channels)


def _plan(rt, name, channels, **kw):
    hw, levels, _, _ = _case(name, channels)
    plan = rt.PyramidPlan(hw[0], hw[1], channels, levels, **kw)
    if not kw:
        assert (plan.streamable, plan.walk_plans) == pg.ROUTES[name][0 if channels == 1 else 1], name
    return plan


# ----------------------------------------------------------------------------- against the oracle

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_plan_run_against_the_oracle(rt, name, channels):
    hw, levels, frames, want = _case(name, channels)
    plan = _plan(rt, name, channels)
    got = _levels_of(plan.run(frames), 2, levels, channels)
    pg.assert_levels_close(got, want, "plan geometry c%d %s" % (channels, _route(name, channels)))
    for g, lv in zip(got, levels):           # uncovered canvas, dead rows / columns: exactly 0
        assert not g[pg.zero_mask(lv)].any(), (name, lv)
    plan.close()


def _outside(lv, hw):
    """Frame pixels one pixel outside a level's crop (edges and corners), as far as the frame has them."""
    y0, x0, ch, cw = lv[:4]
    spots = [(y0 - 1, x0 + cw // 2), (y0 + ch, x0 + cw // 3), (y0 + ch // 2, x0 - 1), (y0 + ch // 3, x0 + cw), (y0 - 1, x0 - 1),
             (y0 + ch, x0 + cw), (y0 - 1, x0 + cw), (y0 + ch, x0 - 1), (y0 - 1, x0), (y0 + ch - 1, x0 + cw)]
    return [(y, x) for y, x in spots if 0 <= y < hw[0] and 0 <= x < hw[1]]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_route_knobs_are_bit_identical(rt, name, channels):
    """The default route against the fallback routes on clean frames and on one with NaN / inf pixels on every crop's corners:
    SILENT_TUNE_PYRAMID 1 (no stream kernel), 2 (unit + region kernels), 8 (border pixels as a launch of their own), 4 set when
    the plan is created (one walk plan per level), and SILENT_TUNE_GRAY 16 (the gray pass without the stream kernel)."""
    hw, levels, frames, _ = _case(name, channels)
    frames = np.concatenate([frames, pg.poisoned_inside(frames[0], levels)[None]])
    plan = _plan(rt, name, channels)
    base = plan.run(frames)
    assert not np.isnan(np.asarray(base.data).reshape(4, -1)[:3]).any()
    for knob in (1, 2, 8):
        with rt.tuning(TUNE_PYRAMID, knob):
            _same_bits(base.data, plan.run(frames).data, "%s c%d PYRAMID knob %d" % (name, channels, knob))
    with rt.tuning(TUNE_PYRAMID, 4):
        per_level = rt.PyramidPlan(hw[0], hw[1], channels, levels)
    if channels == 3 and "walk_union" in _route(name, 3):
        assert per_level.walk_plans[0] in (0, len(levels)), (name, per_level.walk_plans)
    _same_bits(base.data, per_level.run(frames).data, "%s c%d per-level plans" % (name, channels))
    per_level.close()
    if channels == 1:
        cs_k, bank = cw.gray_cs(cw.SEED), cw.gray_bank(4, cw.SEED)
        a = plan.gray_pass(frames, cs_k, bank)
        with rt.tuning(TUNE_GRAY, 16):
            b = plan.gray_pass(frames, cs_k, bank)
        for x, y, m in zip(a, b, ("pyramid", "cs", "end")):
            _same_bits(x.data, y.data, "%s GRAY knob 16 %s" % (name, m))
        _same_bits(a[0].data, base.data, "%s gray_pass pyramid" % name)
    plan.close()


# ----------------------------------------------------------------------------- non-finite pixels

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_nonfinite_pixels_stay_out_of_or_follow_the_oracle_into_a_level(rt, name, channels):
    """Frame 1 + l holds NaN and inf pixels one pixel OUTSIDE the crop of level l: that level must equal the clean frame's bit for
    bit (no tap reads past the crop edge, not even with a weight of 0).  The last frame holds NaN / inf INSIDE every crop, a NaN
    under every dead row / column: the oracle's NaN pattern and infinities, dead rows and uncovered canvas still exactly 0."""
    hw, levels, frames, _ = _case(name, channels)
    clean = frames[0]
    batch = [clean]
    for lv in levels:
        f = clean.copy()
        for k, (y, x) in enumerate(_outside(lv, hw)):
            f[y, x, k % channels] = np.nan if k % 2 == 0 else np.inf
        batch.append(f)
    inside = pg.poisoned_inside(clean, levels)
    batch.append(inside)
    plan = _plan(rt, name, channels)
    got = plan.run(np.stack(batch))
    ref = _levels_of(got, 0, levels, channels)
    assert all(np.isfinite(r).all() for r in ref)
    n_placed = 0
    for l, lv in enumerate(levels):
        n_placed += len(_outside(lv, hw))
        _same_bits(_levels_of(got, 1 + l, levels, channels)[l], ref[l], "%s c%d level %d: pixels outside its crop entered" % (name, channels, l))
    assert n_placed > 0 or all(l[:4] == (0, 0) + hw for l in levels)
    with np.errstate(invalid="ignore", over="ignore"):
        want = pg.oracle_pyramid(inside, levels)
    g_in = _levels_of(got, len(batch) - 1, levels, channels)
    assert any(np.isnan(w).any() for w in want)
    pg.assert_levels_close(g_in, want, "plan geometry c%d non-finite" % channels)
    for g, lv in zip(g_in, levels):
        assert not _bits(g[pg.zero_mask(lv)]).any(), (name, lv)
    plan.close()


# ----------------------------------------------------------------------------- the gray pass

def _gray(K):
    return cw.gray_cs(cw.SEED), cw.gray_bank(K, cw.SEED)


def _parts(rt, plan, frames, cs_k, bank, K, parts_seq):
    """silent_gray_pass_parts_dev on poisoned device buffers."""
    import torch
    from pysilent_amd import _lib
    n, px = len(frames), plan.frame_px
    fr = torch.from_numpy(np.array(frames, np.float32)).cuda(0)
    k_cs, k_end = np.ascontiguousarray(cs_k, np.float32), np.ascontiguousarray(bank, np.float32)
    p = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
    c = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
    e = torch.full((n * px * K,), -7.0, dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for parts in parts_seq:
        plan.ctx.check(_lib.load().silent_gray_pass_parts_dev(
            plan.ctx.handle, plan.handle, C.c_void_p(fr.data_ptr()), n, C.c_void_p(k_cs.ctypes.data), C.c_void_p(k_end.ctypes.data), K,
            255.0, C.c_void_p(p.data_ptr()), C.c_void_p(c.data_ptr()), C.c_void_p(e.data_ptr()), parts, C.c_void_p(s)))
    torch.cuda.synchronize()
    return p.cpu().numpy(), c.cpu().numpy(), e.cpu().numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", NAMES)
def test_gray_pass_promises(rt, name, K):
    """include/silent_hip.h: the pyramid of silent_gray_pass is silent_pyramid's, its CS and end maps are silent_gray_line_end's on
    that pyramid, parts 1 then 2 are parts 3 -- bit for bit; float16 storage is the float16 cast of the float32 maps."""
    hw, levels, frames, _ = _case(name, 1)
    cs_k, bank = _gray(K)
    plan = _plan(rt, name, 1)
    pyr, cs, end = plan.gray_pass(frames, cs_k, bank)
    pyr2 = plan.run(frames)
    cs2, end2 = rt.gray_line_end(pyr2, cs_k, bank)
    for a, b, m in ((pyr, pyr2, "pyramid"), (cs, cs2, "cs"), (end, end2, "end")):
        _same_bits(a.data, b.data, "%s K=%d %s" % (name, K, m))
    whole, halves = _parts(rt, plan, frames, cs_k, bank, K, [3]), _parts(rt, plan, frames, cs_k, bank, K, [1, 2])
    for a, b, ref, m in zip(whole, halves, (pyr, cs, end), ("pyramid", "cs", "end")):
        _same_bits(a, np.asarray(ref.data).reshape(-1), "%s K=%d %s: device form" % (name, K, m))
        _same_bits(a, b, "%s K=%d %s: parts 1 + 2 differ from parts 3" % (name, K, m))
    p16, cs16, end16 = plan.gray_pass(frames, cs_k, bank, storage="float16")
    _same_bits(p16.data, pyr.data, "%s K=%d float16 pyramid" % (name, K))
    with np.errstate(over="ignore"):
        for a, b in ((cs16, cs), (end16, end)):
            assert a.data.dtype == np.float16
            np.testing.assert_array_equal(np.asarray(a.data).view(np.uint16), np.asarray(b.data, np.float32).astype(np.float16).view(np.uint16))
    plan.close()


def _ordered(a):
    """float32 -> integers in value order: a difference of 1 is one ulp."""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


@pytest.mark.parametrize("name", NAMES)
def test_gray_pass_float64_accumulation(rt, name):
    """SILENT_PLAN_ACCUM_F64: the pyramid bit-identical to the oracle's or within the 1 ulp the header allows (two float64 sums, one
    more rounding near a midpoint); CS and end bit-identical to the oracle applied to the GPU's own pyramid."""
    import c_oracle as co
    hw, levels, frames, want = _case(name, 1)
    K = KS[NAMES.index(name) % 3]
    cs_k, bank = _gray(K)
    plan = _plan(rt, name, 1, accumulation="float64")
    pyr, cs, end = plan.gray_pass(frames, cs_k, bank)
    _same_bits(pyr.data, plan.run(frames).data, "%s float64 pyramid: gray_pass vs run" % name)
    k_cs, k_end = np.ascontiguousarray(cs_k, np.float32), np.ascontiguousarray(bank, np.float32)
    got = _levels_of(pyr, 2, levels, 1)
    for l, (g, w) in enumerate(zip(got, want)):
        assert int(np.abs(_ordered(g) - _ordered(w)).max()) <= 1, "%s level %d: more than 1 ulp from the oracle" % (name, l)
    for f in (0, 2):
        for l, lev in enumerate(_levels_of(pyr, f, levels, 1)):
            w_cs, w_end = co.gray_line_end_level(np.ascontiguousarray(lev)[None], k_cs, k_end, 255.0)
            _same_bits(_levels_of(cs, f, levels, 1)[l], w_cs[0], "%s float64 cs level %d" % (name, l))
            _same_bits(_levels_of(end, f, levels, K)[l], w_end[0], "%s float64 end level %d" % (name, l))
    plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_gray_keypoints(rt, name):
    """silent_gray_keypoints: the maps of silent_gray_pass bit for bit; the keypoints of tests/gray_kp_oracle.py on the downloaded
    end map."""
    from gray_kp_oracle import gray_tail
    hw, levels, frames, _ = _case(name, 1)
    K = KS[(NAMES.index(name) + 1) % 3]
    selection = NAMES.index(name) % 2 == 0
    cs_k, bank = _gray(K)
    plan = _plan(rt, name, 1)
    pyr, cs, end = plan.gray_pass(frames, cs_k, bank)
    p2, cs2, end2, idx, counts = plan.gray_keypoints(frames, cs_k, bank, selection=selection)
    for a, b, m in ((pyr, p2, "pyramid"), (cs, cs2, "cs"), (end, end2, "end")):
        _same_bits(a.data, b.data, "%s gray_keypoints %s" % (name, m))
    for f in range(len(frames)):
        rows, _, _ = gray_tail(_levels_of(end2, f, levels, K), pad=2, selection=selection, top_percent=0.1)
        assert counts[f] == len(rows), (name, f, counts[f], len(rows))
        np.testing.assert_array_equal(np.asarray(idx)[f, :counts[f]], rows, err_msg="%s frame %d" % (name, f))
    plan.close()


# ----------------------------------------------------------------------------- random plans

@pytest.mark.parametrize("seed", pg.RANDOM_SEEDS)
def test_random_plans_against_the_oracle(rt, seed):
    hw, channels, levels = pg.random_case(seed)
    frames = pg.frames_of(hw, channels, 3, seed=100 + seed)
    want = pg.oracle_pyramid(frames[-1], levels)
    plan = rt.PyramidPlan(hw[0], hw[1], channels, levels)
    pyr = plan.run(frames)
    got = _levels_of(pyr, 2, levels, channels)
    pg.assert_levels_close(got, want, "plan geometry random c%d" % channels)
    for g, lv in zip(got, levels):
        assert not g[pg.zero_mask(lv)].any(), (seed, lv)
    with rt.tuning(TUNE_PYRAMID, 2):
        _same_bits(pyr.data, plan.run(frames).data, "random %d: unit + region kernels" % seed)
    if channels == 1:
        import err_bound as eb
        from conftest import assert_close
        K = KS[seed % 3]
        cs_k, bank = _gray(K)
        p2, cs, end = plan.gray_pass(frames, cs_k, bank)
        _same_bits(p2.data, pyr.data, "random %d: gray_pass pyramid" % seed)
        cs2, end2 = rt.gray_line_end(pyr, cs_k, bank)
        _same_bits(cs.data, cs2.data, "random %d: cs" % seed)
        _same_bits(end.data, end2.data, "random %d: end" % seed)
        import silent_oracle as so
        for l, w in enumerate(want):
            w_cs, w_end = so.gray_line_end_pass([w[None]], cs_k, bank)[0]
            e_pyr = eb.zoom(w[None])
            e_cs, e_end = eb.gray_chain(w[None], cs_k, bank, w_cs, e_pyr)
            assert_close(_levels_of(cs, 2, levels, 1)[l][None], w_cs, 1e-5, scale=255.0, what="cs plan geometry random", bound=e_cs)
            assert_close(_levels_of(end, 2, levels, K)[l][None], w_end, 1e-5, scale=255.0, what="end plan geometry random", bound=e_end)
    plan.close()
