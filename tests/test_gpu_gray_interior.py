"""In the K = 4 instantiations with up to four general levels (kStreamTwoBodies) a wave of gray_stream_kernel takes one of two bodies:
the INTERIOR body (no mirror clamps, no row / column predicates, no padding selects) where its 25 stream rows and 65 columns lie inside
the crop, the zoom and the level, and the general body elsewhere (csrc/silent_gray.h: gray_stream_tile).  Both must write what the
two-step path -- unit-fused + region + filter kernels, untouched by that split -- writes, bit for bit.  The families with K = 3, K = 8
or seven general levels run the one-body kernels on the same shapes.

Shapes: the smallest at which the split can go wrong, derived from the kernel's predicate (interior_waves below restates it; tiles
are 16 rows, waves 56 columns, blocks 4 waves): no interior wave, exactly one, interior waves next to edge waves in both directions
and in two block columns, interior tile rows above a partial last tile row.  Frame 1 of every float batch holds a NaN, a +inf and
a -inf where an interior wave's halo (first stream row / first lane, last stream row / last lane, the edge column) reads them, frame
2 where the general body's mirror reads them (one pixel inside the frame's corners)."""
import numpy as np
import pytest

import chain_weights as cw
import plan_geometry as pg
import write_coverage as wc
from pysilent_amd._lib import TUNE_GRAY

TH, COLS, BLOCK_WAVES = 16, 56, 4


def interior_waves(lv):
    """[(tile row, wave column)] of the interior waves of a unit level (src_y0, src_x0, src_h, src_w, zoom_h, zoom_w, out_h, out_w)."""
    lim_h, lim_w = min(lv[2], lv[4], lv[6]), min(lv[3], lv[5], lv[7])
    return [(ty, wx) for ty in range(-(-lv[6] // TH)) for wx in range(-(-lv[7] // COLS))
            if ty * TH >= 4 and ty * TH + TH + 4 < lim_h and wx * COLS >= 4 and wx * COLS + 60 < lim_w]


# frame (H, W) -> the interior waves it is chosen for
SHAPES = {
    (36, 116): [],
    (37, 117): [(1, 1)],
    (53, 229): [(ty, wx) for ty in (1, 2) for wx in (1, 2, 3)],
    (53, 285): [(ty, wx) for ty in (1, 2) for wx in (1, 2, 3, 4)],            # wave column 4: the second block column
    (70, 300): [(ty, wx) for ty in (1, 2, 3) for wx in (1, 2, 3, 4)],         # tile row 4 holds the last 6 rows
}
BOTH = [(37, 117), (70, 300)]

# family -> K, ladder (ratio, general levels), plan / call keywords, value range of the frames
FAMILIES = {
    "k3": dict(K=3),
    "k4": dict(K=4),
    "k8": dict(K=8),
    "float16": dict(K=4, call=dict(storage="float16")),
    "float64": dict(K=4, plan=dict(accumulation="float64")),
    "keypoints": dict(K=4, keypoints=True),
    "uint8": dict(K=4, call=dict(frame_dtype="uint8"), dtype=np.uint8),
    "uint16": dict(K=4, call=dict(frame_dtype="uint16", clip_hi=4095.0), dtype=np.uint16, top=4095),
    "strided": dict(K=4, call=dict(frame_dtype="uint8", frame_layout="strided"), dtype=np.uint8, strided=True),
    "dense": dict(K=4, ladder=(2 ** .5, 7)),                                   # slot layout 1: five rows of the first level in flight
}
# a plan of tests/plan_geometry.py whose unit level has a canvas wider than its zoom: col_eff differs from col_in
CANVAS_CASE = "ucanvas_tl_316"


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _levels(hw, fam):
    if hw == CANVAS_CASE:
        return pg.CASES[CANVAS_CASE]["frame"], pg.CASES[CANVAS_CASE]["levels"]
    ratio, n = FAMILIES[fam].get("ladder", (pg.E, 2))
    return hw, pg.ladder((0, 0) + hw, ratio, n)


def _poison(frames, unit):
    """NaN / +inf / -inf into frames 1 (an interior wave's halo) and 2 (the mirror of the edge waves), inside the unit level's crop."""
    y0, x0, ch, cw_ = unit[:4]
    ty, wx = (interior_waves(unit) or [(1, 1)])[0]
    ry, rx = ty * TH, wx * COLS
    for (y, x), v in zip(((ry - 4, rx - 4), (ry + TH + 4, rx + 59), (ry + TH // 2, rx + 60)), (np.nan, np.inf, -np.inf)):
        frames[1, y0 + min(y, ch - 1), x0 + min(x, cw_ - 1), 0] = v
    for (y, x), v in zip(((1, 1), (ch - 2, cw_ - 2), (0, cw_ // 2)), (np.nan, np.inf, -np.inf)):
        frames[2, y0 + y, x0 + x, 0] = v


_CACHE = {}


def _case(hw, fam):
    """(frame hw, levels, frames [3, H, W, 1] as the family's dtype): made once, never modified."""
    key = (hw, fam)
    if key not in _CACHE:
        f = FAMILIES[fam]
        fhw, levels = _levels(hw, fam)
        assert pg.is_valid(fhw, levels) and pg.stream_layout(levels) == (1 if "ladder" in f else 0), (hw, fam)
        rng = np.random.default_rng(5200 + 31 * fhw[1] + sorted(FAMILIES).index(fam))
        frames = rng.integers(0, f.get("top", 255) + 1, (3,) + fhw + (1,)).astype(f.get("dtype", np.float32))
        if frames.dtype == np.float32:
            _poison(frames, next(l for l in levels if pg.is_unit(l)))
        frames.setflags(write=False)
        _CACHE[key] = (fhw, levels, frames)
    return _CACHE[key]


def _on_device(frames, fam):
    import torch
    if not FAMILIES[fam].get("strided"):
        return torch.from_numpy(np.array(frames)).cuda(0)
    n, h, w, _ = frames.shape
    big = torch.full((n, h + 11, w + 37, 1), 77, dtype=torch.uint8, device="cuda:0")      # pitch and offsets of no particular alignment
    view = big[:, 7:7 + h, 5:5 + w]
    view.copy_(torch.from_numpy(np.array(frames)).cuda(0))
    return view


def _run(rt, plan, x, fam):
    """The family's call -> (pyramid, cs, end[, Rows])."""
    f = FAMILIES[fam]
    cs_k, bank = cw.gray_cs(cw.SEED), cw.gray_bank(f["K"], cw.SEED)
    kw = dict(f.get("call", {}))
    if f.get("keypoints"):
        pyr, cs, end, idx, counts = plan.gray_keypoints(x, cs_k, bank, **kw)
        return [pyr, cs, end, wc.Rows(idx, counts)]
    return list(plan.gray_pass(x, cs_k, bank, **kw))


def _split(packed, f, levels, channels):
    return pg.split(wc.to_numpy(packed.data).reshape(packed.n_frames, -1)[f], levels, channels)


def test_the_shapes_have_the_interior_waves_they_are_chosen_for():
    for hw, want in SHAPES.items():
        unit = pg.ladder((0, 0) + hw, pg.E, 2)[0]
        assert interior_waves(unit) == want, hw
    assert SHAPES[(70, 300)] and 70 % TH and max(wx for _, wx in SHAPES[(53, 285)]) >= BLOCK_WAVES > max(wx for _, wx in SHAPES[(53, 229)])
    unit = pg.CASES[CANVAS_CASE]["levels"][0]
    assert pg.is_unit(unit) and unit[5] < unit[7] and interior_waves(unit)
    assert any(wx * COLS + 60 >= unit[5] > wx * COLS for wx in range(-(-unit[7] // COLS)))       # and a wave that straddles the zoom's edge


CASES = [(hw, "k4") for hw in SHAPES if hw not in BOTH] + [(hw, fam) for fam in FAMILIES for hw in BOTH] + [(CANVAS_CASE, "k4")]
IDS = ["%s-%s" % (hw if isinstance(hw, str) else "%dx%d" % hw, fam) for hw, fam in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("hw,fam", CASES, ids=IDS)
def test_stream_path_equals_the_two_step_path(rt, hw, fam):
    """Pyramid, CS and end maps (and the keypoint rows) of the stream kernel against SILENT_TUNE_GRAY 16, bit for bit, NaNs in place."""
    fhw, levels, frames = _case(hw, fam)
    plan = rt.PyramidPlan(fhw[0], fhw[1], 1, levels, **FAMILIES[fam].get("plan", {}))
    assert plan.streamable
    x = _on_device(frames, fam)
    got = wc.specified(_run(rt, plan, x, fam))
    with rt.tuning(TUNE_GRAY, 16):
        want = wc.specified(_run(rt, plan, x, fam))
    plan.close()
    if frames.dtype == np.float32:
        assert np.isnan(got[0][1]).any() and np.isinf(got[0][1]).any()
    wc.assert_same_bits(got, want, "%s %s: stream against two-step" % (hw, fam))


ORACLE = [((70, 300), fam) for fam in FAMILIES] + [(CANVAS_CASE, "k4")]


@pytest.mark.gpu
@pytest.mark.parametrize("hw,fam", ORACLE, ids=["%s-%s" % (hw if isinstance(hw, str) else "%dx%d" % hw, fam) for hw, fam in ORACLE])
def test_stream_path_against_the_oracle(rt, hw, fam):
    """One case per family against the C oracle per level: the project's range-relative 1e-5 and the element-wise rounding bound of
    tests/err_bound.py (frames 0, clean, and 2, NaN / inf under the mirror).  float16 storage: the float16 cast of the float32 maps of
    the same call, bit for bit -- those are what the "k4" case holds against the oracle.  Keypoints: tests/gray_kp_oracle.py on the
    downloaded end map of the clean frame."""
    import err_bound as eb
    import silent_oracle as so
    from conftest import assert_close
    f = FAMILIES[fam]
    fhw, levels, frames = _case(hw, fam)
    K, scale = f["K"], float(f.get("top", 255))
    cs_k, bank = cw.gray_cs(cw.SEED), cw.gray_bank(K, cw.SEED)
    plan = rt.PyramidPlan(fhw[0], fhw[1], 1, levels, **f.get("plan", {}))
    assert plan.streamable
    x = _on_device(frames, fam)
    res = _run(rt, plan, x, fam)
    pyr, cs, end = res[:3]
    if fam == "float16":
        _, cs32, end32 = plan.gray_pass(x, cs_k, bank)
        with np.errstate(over="ignore"):
            for a, b, m in ((cs, cs32, "cs"), (end, end32, "end")):
                assert wc.to_numpy(a.data).dtype == np.float16
                np.testing.assert_array_equal(wc.to_numpy(a.data).view(np.uint16), wc.to_numpy(b.data).astype(np.float16).view(np.uint16), err_msg=m)
        cs, end = cs32, end32
    plan.close()
    clip_hi = f.get("call", {}).get("clip_hi", 255.0)
    for fr in (0, 2):
        with np.errstate(invalid="ignore", over="ignore"):
            want = pg.oracle_pyramid(np.asarray(frames[fr], np.float32), levels)
        for l, w in enumerate(want):
            tag = "%s %s frame %d level %d" % (hw, fam, fr, l)
            with np.errstate(invalid="ignore", over="ignore"):
                w_cs, w_end = so.gray_line_end_pass([w[None]], cs_k, bank, clip_hi=clip_hi)[0]
                e_pyr = eb.zoom(w[None])
                e_cs, e_end = eb.gray_chain(w[None], cs_k, bank, w_cs, e_pyr)
            assert_close(_split(pyr, fr, levels, 1)[l][None], w[None], 1e-5, scale=scale, what="pyramid " + tag, bound=e_pyr)
            assert_close(_split(cs, fr, levels, 1)[l][None], w_cs, 1e-5, scale=scale, what="cs " + tag, bound=e_cs)
            assert_close(_split(end, fr, levels, K)[l][None], w_end, 1e-5, scale=scale, what="end " + tag, bound=e_end)
    if f.get("keypoints"):
        from gray_kp_oracle import gray_tail
        idx, counts = wc.to_numpy(res[3].idx), wc.to_numpy(res[3].counts)
        rows, _, _ = gray_tail(_split(end, 0, levels, K), pad=2, selection=True, top_percent=0.1)
        assert counts[0] == len(rows)
        np.testing.assert_array_equal(idx[0, :counts[0]], rows)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,fam", CASES, ids=IDS)
def test_stream_path_writes_all_of_its_output_and_nothing_else(rt, monkeypatch, hw, fam):
    """The canaries of tests/write_coverage.py: results between guards under two fills (and once at the weakest alignment the header
    allows): no guard byte touched, no element that follows the fill -- a wrong store mask or row pointer of either body shows here."""
    fhw, levels, frames = _case(hw, fam)
    plan = rt.PyramidPlan(fhw[0], fhw[1], 1, levels, **FAMILIES[fam].get("plan", {}))
    x = _on_device(frames, fam)
    base = wc.specified(_run(rt, plan, x, fam))
    got = []
    for fill, lead in [(fl, 0) for fl in wc.FILLS] + [(wc.FILLS[0], wc.weakest_alignment)]:
        what = "%s %s, fill 0x%02X%s" % (hw, fam, fill, ", weakest alignment" if lead else "")
        with wc.guarded(rt, monkeypatch, fill, lead) as gb:
            raw = _run(rt, plan, x, fam)
        for t in wc.buffers_of(raw):
            assert gb.owns(t), what
        got.append(wc.specified(raw))
        gb.check(what)
        wc.assert_same_bits(got[-1], base, what + " against an ordinary run")
    wc.assert_same_bits(got[1], got[0], "%s %s: fill 0x5A against fill 0xA5" % (hw, fam))
    plan.close()
