"""The fused keypoint calls -- silent_gray_keypoints* and silent_rgb_keypoints[_h] -- away from pad = 2 and regions = half the level,
the one point of their argument space the rest of the suite runs them at (tests/kp_regions.py: families, pads, geometries, frames;
tests/test_kp_regions.py shows on the CPU that these inputs take the paths and give the different rows they are chosen for).

Everything is compared bit for bit: rows and counts with np.array_equal, maps as integers with NaNs in place.  Per case the maps are
those of the maps-only step, rows / counts / value maps those of the GPU per-op composite on the same end map, and the rows those of
the oracle's tail (tests/gray_kp_oracle.py, oracle/silent_oracle.py) on the downloaded map."""
import numpy as np
import pytest

import kp_regions as kr
import silent_oracle as so
import write_coverage as wc
from gray_kp_oracle import gray_tail
from test_gray_keypoints import _check_against_composite, _pipe, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda(0)


def _assert_rows(got, want, what):
    assert np.array_equal(got["keypoint_counts"], want["keypoint_counts"]), (what, got["keypoint_counts"], want["keypoint_counts"])
    for f, (a, b) in enumerate(zip(got["keypoints"], want["keypoints"])):
        assert np.array_equal(a, b), "%s: rows of frame %d differ" % (what, f)


# ----------------------------------------------------------------------------- gray

def _gray_cases():
    cases = []

    def add(*c):
        if c not in cases:
            cases.append(c)
    for fam in kr.FAMILIES:                                             # every family at pad 2
        add("G3" if fam == "unit" else "G1", fam, 2, 4, 0.1, 255.0)
    for pad in kr.PADS:                                                 # every pad on a cell-table, the last cell-table and a general family
        for fam in ("default", "four", "cells3"):
            add("G1", fam, pad, 4, 0.1, 255.0)
    for fam in ("four", "five_rows"):                                   # the reference's crop layout
        for pad in (0, 3):
            add("G2", fam, pad, 4, 0.1, 255.0)
    for K in (3, 8):                                                    # the other channel counts of the selection kernels
        for fam in ("four", "five_cols"):
            for pad in (0, 3):
                add("G1", fam, pad, K, 0.1, 255.0)
    for p in (0.0, 1.0):                                                # thresholds at the level maximum / minimum
        for pad in (0, "big"):
            for fam in ("default", "cells3"):
                add("G1", fam, pad, 4, p, 255.0)
    for fam in ("four", "cells3"):                                      # a saturated end map: plateaus of ties at the maximum
        add("G1", fam, 2, 4, 0.1, 8.0)
    return cases


GRAY_CASES = _gray_cases()
GRAY_IDS = ["%s-%s-pad%s-K%d-p%g-clip%g" % c for c in GRAY_CASES]


def _ends(out, batch, n_levels):
    return [[out["end"].level(l)[f].cpu().numpy() for l in range(n_levels)] for f in range(batch)]


def _gray_case(rt, geo, fam, pad, K, top_percent, clip_hi, frames, n_frames=kr.N_FRAMES, widened=None, extra={}, ref_extra={}):
    """One (geometry, family, pad, K, top_percent, clip_hi) against the maps-only step, the per-op composite, the oracle's tail and --
    sparse tail -- the dense kernels, for selection on / off and with / without the value and peak-value maps."""
    from pysilent_amd._lib import TUNE_GRAY
    g = kr.GEOMETRIES[geo]
    hw, ext = g["hw"], kr.extents(geo)
    regions, p = kr.regions(fam, ext), kr.pad_of(pad, ext)
    which = kr.path(ext, regions)[0]
    ref = _pipe(hw, K, n_frames, False, clip_hi=clip_hi, **dict(g["geo"], **ref_extra))
    assert list(ref.extents) == ext
    ref.step(frames if widened is None else widened)
    want = ref.outputs()
    ends = _ends(want, n_frames, len(ext))
    for selection in (True, False):
        with np.errstate(invalid="ignore", over="ignore"):
            tails = [gray_tail(e, p, selection, top_percent, regions) for e in ends]
        for f, (rows, _, _) in enumerate(tails):
            assert (rows[:, 0] == 0).any(), "frame %d has no row on level 0" % f
        for maps in (True, False):
            what = "%s %s pad %d K %d selection %s maps %s" % (geo, fam, p, K, selection, maps)
            kw = dict(selection=selection, top_percent=top_percent, pad=p, regions=regions, clip_hi=clip_hi, value_map=maps,
                      peak_value_map=maps and selection, **dict(g["geo"], **extra))
            pipe = _pipe(hw, K, n_frames, True, **kw)
            pipe.step(frames)
            out = pipe.outputs()
            stats = pipe.sparse_tail_stats()
            assert ("value" in out) == maps and ("peak_value" in out) == (maps and selection), what
            for k in ("pyramid", "cs", "end"):
                assert _same(out[k].data, want[k].data), "%s: %s differs from the maps-only step" % (what, k)
            counts = _check_against_composite(rt, pipe, out, selection, top_percent)
            for f, (rows, _, _) in enumerate(tails):
                assert counts[f] == len(rows), "%s: frame %d: %d rows, the oracle's tail has %d" % (what, f, counts[f], len(rows))
                assert np.array_equal(out["keypoints"][f], rows), "%s: frame %d: rows differ from the oracle's tail" % (what, f)
            if pad == "big" and not selection:
                # the emptied level: no value but 0 (or NaN) is left, and it contributes what the oracle says -- every pixel that is no NaN
                for f, (rows, values, _) in enumerate(tails):
                    last = values[-1]
                    assert not np.nan_to_num(last, nan=0.0).any(), what
                    n_last = int((rows[:, 0] == len(ext) - 1).sum())
                    assert n_last == int((~np.isnan(last)).sum()) > 0
                    assert int((out["keypoints"][f][:, 0] == len(ext) - 1).sum()) == n_last, what
            if selection and not maps:
                assert stats["ran"] == (which == "cells"), (what, stats)
                # Which (frame, level)s the sparse tail hands to the dense kernels: one with a NaN and a window without a positive
                # peak (frame 3 under "default" at the default pad and threshold; a single window, "one", has its peak), and every
                # level of a frame with more passers than the candidate list holds (top_percent = 1: every pixel passes)
                if fam == "default" and n_frames == kr.N_FRAMES and (pad, top_percent) == (2, 0.1):
                    assert stats["dense_pairs"] >= 1, (what, stats)
                if which == "cells" and top_percent == 1.0:
                    assert sum(h * w for h, w in ext) > 16384 and stats["dense_pairs"] == stats["pairs"] == n_frames * len(ext), (what, stats)
                with rt.tuning(TUNE_GRAY, 64):                              # the dense kernels for every level
                    dense = _pipe(hw, K, n_frames, True, **kw)
                    dense.step(frames)
                    d = dense.outputs()
                    assert not dense.sparse_tail_stats()["ran"]
                _assert_rows(d, out, what + ": dense kernels against the default route")
    return want


@pytest.mark.parametrize("geo,fam,pad,K,top_percent,clip_hi", GRAY_CASES, ids=GRAY_IDS)
def test_gray_keypoints_on_other_pads_and_regions(rt, geo, fam, pad, K, top_percent, clip_hi):
    frames = _dev(kr.frames(kr.GEOMETRIES[geo]["hw"], 1))
    _gray_case(rt, geo, fam, pad, K, top_percent, clip_hi, frames)


def test_the_case_table_is_the_issues():
    got = {(c[0], c[1], c[2]) for c in GRAY_CASES}
    assert {("G1", f, 2) for f in kr.FAMILIES if f != "unit"} | {("G3", "unit", 2)} <= got
    assert {("G1", f, p) for f in ("default", "four", "cells3") for p in kr.PADS} <= got
    assert {c[3] for c in GRAY_CASES} == {3, 4, 8} and {c[4] for c in GRAY_CASES} == {0.0, 0.1, 1.0}


@pytest.mark.parametrize("pad", [0, 2, "big"])
@pytest.mark.parametrize("selection", [True, False])
def test_mixed_levels_but_the_last_are_those_of_default(rt, selection, pad):
    """One (1, 1) level sends the whole call down the general path: the other levels must give what the cell tables give."""
    g = kr.GEOMETRIES["G1"]
    ext = kr.extents("G1")
    frames = _dev(kr.frames(g["hw"], 1))
    rows = {}
    for fam in ("default", "mixed"):
        pipe = _pipe(g["hw"], 4, kr.N_FRAMES, True, selection=selection, pad=kr.pad_of(pad, ext), regions=kr.regions(fam, ext), **g["geo"])
        pipe.step(frames)
        rows[fam] = pipe.outputs()["keypoints"]
        assert pipe.sparse_tail_stats()["ran"] == (selection and fam == "default")
    last = len(ext) - 1
    for f in range(kr.N_FRAMES):
        a, b = rows["default"][f], rows["mixed"][f]
        assert len(a) and np.array_equal(a[a[:, 0] != last], b[b[:, 0] != last]), "frame %d" % f


def _u8_frames(hw):
    """Frames 0 .. 2 as uint8 (the quantised frame's 256 becomes 255), as a pitched view of a larger surface, and widened."""
    import torch
    f = np.minimum(kr.frames(hw, 1)[:3], 255.0).astype(np.uint8)
    n, h, w, _ = f.shape
    big = torch.full((n, h + 11, w + 37, 1), 77, dtype=torch.uint8, device="cuda:0")
    view = big[:, 7:7 + h, 5:5 + w]
    view.copy_(torch.from_numpy(f).cuda(0))
    assert not view.is_contiguous()
    return view, _dev(f.astype(np.float32))


@pytest.mark.parametrize("fam", ["four", "five_cols"])
def test_gray_keypoints_of_a_pitched_uint8_view(rt, fam):
    """frame_dtype="uint8", frame_layout="strided": rows, counts and maps are the float32 pipeline's on the widened frames (the maps
    of the float32 maps-only step, the composite and the oracle's tail on them)."""
    view, wide = _u8_frames(kr.GEOMETRIES["G1"]["hw"])
    _gray_case(rt, "G1", fam, 3, 4, 0.1, 255.0, view, n_frames=3, widened=wide, extra=dict(frame_dtype="uint8", frame_layout="strided"))


def test_gray_keypoints_with_float64_accumulation(rt):
    frames = _dev(kr.frames(kr.GEOMETRIES["G1"]["hw"], 1))
    acc = dict(accumulation="float64")
    _gray_case(rt, "G1", "cells3", 1, 4, 0.1, 255.0, frames, extra=acc, ref_extra=acc)


@pytest.mark.parametrize("fam", ["four", "five_cols"])
@pytest.mark.parametrize("selection", [True, False])
def test_host_form_equals_the_device_pipeline(rt, selection, fam):
    """PyramidPlan.gray_keypoints on NumPy frames (silent_gray_keypoints: staged, no value maps from the caller)."""
    g = kr.GEOMETRIES["G1"]
    ext = kr.extents("G1")
    regions = kr.regions(fam, ext)
    frames = kr.frames(g["hw"], 1)
    pipe = _pipe(g["hw"], 4, kr.N_FRAMES, True, selection=selection, pad=3, regions=regions, **g["geo"])
    pipe.step(_dev(frames))
    out = pipe.outputs()
    pyr, cs, end, idx, counts = pipe.plan.gray_keypoints(np.array(frames), pipe.consts["cs"], pipe.consts["end"], pad=3,
                                                         selection=selection, top_percent=0.1, regions=regions)
    assert np.array_equal(counts, out["keypoint_counts"])
    for f in range(kr.N_FRAMES):
        assert counts[f] > 0 and np.array_equal(idx[f, :counts[f]], out["keypoints"][f]), "frame %d" % f
    wc.assert_same_bits([(n, m) for n, m in zip(("pyramid", "cs", "end"), (pyr, cs, end))],
                        [(n, out[n]) for n in ("pyramid", "cs", "end")], "host form against the device pipeline")


def test_a_capacity_below_the_count_on_the_general_path(rt):
    g = kr.GEOMETRIES["G1"]
    ext = kr.extents("G1")
    regions = kr.regions("five_cols", ext)
    frames = _dev(kr.frames(g["hw"], 1))
    full = _pipe(g["hw"], 4, kr.N_FRAMES, True, selection=False, pad=1, regions=regions, **g["geo"])
    full.step(frames)
    want = full.outputs()
    cap = int(want["keypoint_counts"].min()) // 2
    assert cap > 0
    pipe = _pipe(g["hw"], 4, kr.N_FRAMES, True, selection=False, pad=1, regions=regions, max_keypoints_per_frame=cap, **g["geo"])
    pipe.step(frames)
    with pytest.raises(ValueError, match="capacity"):
        pipe.outputs()
    out = pipe.outputs(allow_truncated=True)
    assert np.array_equal(out["keypoint_counts"], want["keypoint_counts"])
    for f in range(kr.N_FRAMES):
        assert np.array_equal(out["keypoints"][f], want["keypoints"][f][:cap])


@pytest.mark.parametrize("selection", [False, True])
def test_general_path_writes_all_of_its_output_and_nothing_else(rt, monkeypatch, selection):
    """The canaries of tests/write_coverage.py around plan.gray_keypoints with "five_cols": the value map (selection off) or the
    peak-value map (on) lives in the context workspace next to the general path's row and window maxima."""
    g = kr.GEOMETRIES["G1"]
    ext = kr.extents("G1")
    regions = kr.regions("five_cols", ext)
    frames = _dev(kr.frames(g["hw"], 1))
    plan = rt.PyramidPlan(g["hw"][0], g["hw"][1], 1, kr.levels("G1"))
    from pysilent_amd.pipeline import default_constants
    k = default_constants("gray", 4)

    def run():
        pyr, cs, end, idx, counts = plan.gray_keypoints(frames, k["cs"], k["end"], pad=3, selection=selection, regions=regions)
        return [pyr, cs, end, wc.Rows(idx, counts)]
    base = wc.specified(run())
    got = []
    for fill, lead in [(fl, 0) for fl in wc.FILLS] + [(wc.FILLS[0], wc.weakest_alignment)]:
        what = "five_cols selection %s, fill 0x%02X%s" % (selection, fill, ", weakest alignment" if lead else "")
        with wc.guarded(rt, monkeypatch, fill, lead) as gb:
            raw = run()
        for t in wc.buffers_of(raw):
            assert gb.owns(t), what
        got.append(wc.specified(raw))
        gb.check(what)
        wc.assert_same_bits(got[-1], base, what + " against an ordinary run")
    wc.assert_same_bits(got[1], got[0], "five_cols: fill 0x5A against fill 0xA5")
    plan.close()


# ----------------------------------------------------------------------------- RGB

RGB_CASES = ([("R1", fam, 2) for fam in kr.FAMILIES if fam != "unit"] +
             [("R1", fam, pad) for pad in (0, 1, 3) for fam in ("default", "four", "cells3")] +
             [("R2", fam, 2) for fam in ("four", "five_cols")])


def _rgb_pipe(geo, fam, pad, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    g = kr.GEOMETRIES[geo]
    ext = kr.extents(geo)
    kw.setdefault("selection", True)
    pipe = LineEndPipeline(g["hw"], mode="rgb", batch=kr.N_FRAMES, placement=None, pad=pad, regions=kr.regions(fam, ext), **dict(g["geo"], **kw))
    assert list(pipe.extents) == ext
    return pipe


def _rgb_maps_same(a, b, names, what):
    wc.assert_same_bits([(n, a[n]) for n in names], [(n, b[n]) for n in names], what)


def _rgb_oracle_rows(out, geo, fam, selection):
    """The oracle's tail on the downloaded (already padded) line_end map: one row list per frame."""
    ext = kr.extents(geo)
    regions = kr.regions(fam, ext)
    per_frame = []
    for f in range(kr.N_FRAMES):
        rows = []
        for l, (rh, rw) in enumerate(regions):
            lev = out["line_end"].level(l)[f:f + 1].cpu().numpy()
            with np.errstate(invalid="ignore", over="ignore"):
                v = so.value_from_color(lev)
                if selection:
                    v = so.value_from_color(so.nms3x3(so.top_value_points(lev, 0.1), "product"))
                r = so.max_value_indices_region(None, (1, rh, rw, 3), v)
            r[:, 0] = l
            rows.append(r)
        per_frame.append(np.concatenate(rows).astype(np.int64).reshape(-1, 4))
    return per_frame


@pytest.mark.parametrize("geo,fam,pad", RGB_CASES, ids=["%s-%s-pad%d" % c for c in RGB_CASES])
def test_rgb_keypoints_on_other_pads_and_regions(rt, geo, fam, pad):
    import torch
    from pysilent_amd._lib import TUNE_RGB
    ext = kr.extents(geo)
    which = kr.path(ext, kr.regions(fam, ext))[0]
    t = _dev(kr.frames(kr.GEOMETRIES[geo]["hw"], 3))
    what = "%s %s pad %d" % (geo, fam, pad)
    # the fused step against chain, then selection
    fused, plain = _rgb_pipe(geo, fam, pad), _rgb_pipe(geo, fam, pad)
    fused.step(t)                           # run_pyramid + silent_rgb_keypoints_dev
    plain.run_pyramid(t)
    plain.run_filters()                     # silent_rgb_line_end_dev
    plain.run_keypoints()                   # silent_select_keypoints_dev
    torch.cuda.synchronize()
    a, b = fused.outputs(), plain.outputs()
    _rgb_maps_same(a, b, ("pyramid", "orient", "line_end", "value", "peak_value"), what + ": fused against chain + selection")
    _assert_rows(a, b, what + ": fused against chain + selection")
    # ... and the oracle's tail on the line_end map
    want = _rgb_oracle_rows(a, geo, fam, True)
    for f in range(kr.N_FRAMES):
        assert np.array_equal(a["keypoints"][f], want[f]), "%s: frame %d: rows differ from the oracle's tail" % (what, f)
    assert sum(len(r) for r in want) > 0
    # the sparse tail (no peak-value map) against the dense kernels
    sparse, dense = _rgb_pipe(geo, fam, pad, peak_value_map=False, value_map=False), _rgb_pipe(geo, fam, pad, peak_value_map=False, value_map=False)
    sparse.step(t)
    s = sparse.outputs()
    stats = sparse.sparse_tail_stats()
    assert stats["ran"] == (which == "cells"), (what, stats)
    knob = rt.get_context().get_tuning(TUNE_RGB)
    with rt.tuning(TUNE_RGB, knob | 32):
        dense.step(t)
        d = dense.outputs()
        assert not dense.sparse_tail_stats()["ran"]
    assert "peak_value" not in s and "value" not in s
    _assert_rows(s, a, what + ": sparse tail against the fused step with maps")
    _assert_rows(d, a, what + ": dense kernels against the fused step with maps")
    _rgb_maps_same(s, a, ("orient", "line_end"), what + ": sparse")


@pytest.mark.parametrize("fam", ["four", "cells3"])
def test_rgb_keypoints_without_selection(rt, fam):
    """The reference graph: silent_max_value_indices_region_dev on the value map."""
    t = _dev(kr.frames(kr.GEOMETRIES["R1"]["hw"], 3))
    pipe = _rgb_pipe("R1", fam, 3, selection=False)
    pipe.step(t)
    out = pipe.outputs()
    want = _rgb_oracle_rows(out, "R1", fam, False)
    for f in range(kr.N_FRAMES):
        assert len(want[f]) and np.array_equal(out["keypoints"][f], want[f]), "frame %d" % f


@pytest.mark.parametrize("peak_map", [False, True])
@pytest.mark.parametrize("fam", ["four", "cells3"])
def test_rgb_float16_keypoints_equal_the_pair_of_calls(rt, fam, peak_map):
    """silent_rgb_keypoints_h_dev = silent_rgb_line_end_h_dev + silent_select_keypoints_dev on the widened line_end
    (tests/test_gpu_rgb_float16.py: test_keypoints_equal_the_pair_of_calls) with 4 windows and with 3 x 3 regions: the cell
    tables at their limit and the general path with a float16 colour map."""
    import test_gpu_rgb_float16 as h16
    regions = kr.regions(fam, h16.EXTENTS)
    which = kr.path(h16.EXTENTS, regions)[0]
    assert which == ("cells" if fam == "four" else "general")
    flat, _ = h16._input("noise")
    h, pair, f, st = h16._kp_calls(rt, flat, h16._weights("reference"), 0.1, peak_map, regions=regions)
    h16._assert_same_keypoints(h, pair, "%s map=%s" % (fam, peak_map))
    assert bool(st[0]) == (which == "cells"), st
    assert int(h["counts"].sum()) > 0
