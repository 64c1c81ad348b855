"""The inputs of tests/test_gpu_keypoint_regions.py do what they are chosen for (CPU, oracle only): the region families take the
path they are named for, the pads and families give different keypoint rows on the committed frames (a test that compares rows could
not tell them apart otherwise), and the restatement of region_axis in tests/kp_regions.py agrees with the oracle's windows."""
import itertools

import numpy as np
import pytest

import kp_regions as kr
import silent_oracle as so
from gray_kp_oracle import gray_tail


@pytest.mark.parametrize("geo", ["G1", "G2", "R1", "R2"])
def test_families_take_the_path_they_are_named_for(geo):
    ext = kr.extents(geo)
    for fam in kr.CELLS:
        assert kr.path(ext, kr.regions(fam, ext))[0] == "cells", fam
    for fam in kr.GENERAL:
        assert kr.path(ext, kr.regions(fam, ext))[0] == "general", fam
    _, t = kr.path(ext, kr.regions("five_cols", ext))
    assert all(l["wy"] <= kr.MAX_WIN and l["sy"] <= kr.MAX_SEG for l in t) and any(l["wx"] > kr.MAX_WIN for l in t)
    _, t = kr.path(ext, kr.regions("five_rows", ext))
    assert all(l["wx"] <= kr.MAX_WIN and l["sx"] <= kr.MAX_SEG for l in t) and any(l["wy"] > kr.MAX_WIN for l in t)
    _, t = kr.path(ext, kr.regions("four", ext))
    assert (t[0]["wy"], t[0]["wx"]) == (4, 4)
    # one and over: a single window that is the whole level
    for fam in ("one", "over"):
        for (h, w), l in zip(ext, kr.path(ext, kr.regions(fam, ext))[1]):
            assert l["rows"] == [(0, h)] and l["cols"] == [(0, w)]
    # mixed: only the last level leaves the cell tables
    _, t = kr.path(ext, kr.regions("mixed", ext))
    assert all(max(l["wy"], l["wx"]) <= kr.MAX_WIN for l in t[:-1]) and max(t[-1]["wy"], t[-1]["wx"]) > kr.MAX_WIN


def test_default_has_a_level_with_three_windows():
    for geo in ("G1", "R1"):
        ext = kr.extents(geo)
        _, t = kr.path(ext, kr.regions("default", ext))
        assert any(3 in (l["wy"], l["wx"]) for l in t) and any(2 in (l["wy"], l["wx"]) for l in t), geo


def test_unit_is_general_on_the_small_geometry():
    ext = kr.extents("G3")
    p, t = kr.path(ext, kr.regions("unit", ext))
    assert p == "general" and [(l["wy"], l["wx"]) for l in t] == ext


def test_four_windows_reach_the_most_segments_four_windows_can_have():
    """kMaxSeg = 8 (csrc/silent_peaks.h: "<= 2 * windows") is a bound no table reaches: every window of this pool is the level
    clipped to a shifted copy of itself, window j starts at j * stride - ((out - 1) * stride) // 2, so about half of the windows
    start at 0 and the other half end at the level's end -- out windows give at most out + 1 segments.  Shown here for every extent
    up to 400 and every stride, so 4 windows have at most 5 segments; "four" reaches those 5 on every axis of every level."""
    most = {}
    for size in range(1, 401):
        for stride in range(1, size + 2):
            wins, cuts = kr.axis(size, stride)
            most[len(wins)] = max(most.get(len(wins), 0), len(cuts) - 1)
            assert len(cuts) - 1 <= len(wins) + 1, (size, stride)
    assert most[4] == 5 and most[3] == 3 and most[2] == 3 and most[1] == 1
    for geo in ("G1", "G2", "R1", "R2"):
        ext = kr.extents(geo)
        for l in kr.path(ext, kr.regions("four", ext))[1]:
            assert (l["wy"], l["wx"], l["sy"], l["sx"]) == (4, 4, 5, 5), geo


def test_pads():
    for geo in ("G1", "R1"):
        ext = kr.extents(geo)
        big = kr.big_pad(ext)
        h, w = ext[-1]
        assert 2 * big >= min(h, w) > 2 * (big - 1)                  # the smallest pad that empties the last level
        assert min(ext[0]) > 2 * big + 16                            # level 0 keeps an interior of more than a tile
        assert big not in (0, 1, 2, 3)
    assert kr.pad_of("big", kr.extents("G1")) == 6 and kr.pad_of(3, kr.extents("G1")) == 3


def test_extents_are_the_oracles():
    g = kr.GEOMETRIES["G1"]
    assert kr.extents("G1") == so.classic_extents(g["hw"][0], g["hw"][1], g["geo"]["scale"], g["geo"]["n_levels"])
    g = kr.GEOMETRIES["G2"]
    n = so.ref_num_scales(g["hw"], (32, 48), g["geo"]["scale"])
    assert kr.extents("G2") == [(32, 48)] * n


# ----------------------------------------------------------------------------- the inputs discriminate

@pytest.fixture(scope="module")
def g1_ends():
    """[frame][level] -> [h, w, 4] end map of the oracle on its own pyramid of frames 0 .. 2 of G1 (read-only)."""
    from pysilent_amd.pipeline import default_constants
    g = kr.GEOMETRIES["G1"]
    k = default_constants("gray", 4)
    out = []
    for f in kr.frames(g["hw"], 1)[:3]:
        pyr = so.classic_pyramid(f, g["geo"]["scale"], g["geo"]["n_levels"])
        ends = [e[0] for _, e in so.gray_line_end_pass(pyr, k["cs"], k["end"])]
        for e in ends:
            e.setflags(write=False)
        out.append(ends)
    return out


def _row_sets(ends, pad, selection, regions):
    return [frozenset(map(tuple, gray_tail(e, pad, selection, 0.1, regions)[0])) for e in ends]


@pytest.mark.parametrize("selection", [True, False])
def test_families_and_pads_give_different_rows(g1_ends, selection):
    ext = kr.extents("G1")
    assert [e.shape[:2] for e in g1_ends[0]] == ext
    fams = ("default", "one", "four", "five_cols", "cells3")
    rows = {fam: _row_sets(g1_ends, 2, selection, kr.regions(fam, ext)) for fam in fams}
    for a, b in itertools.combinations(fams, 2):
        assert any(x != y for x, y in zip(rows[a], rows[b])), "%s and %s give the same rows on every frame" % (a, b)
    pads = {p: _row_sets(g1_ends, kr.pad_of(p, ext), selection, kr.regions("default", ext)) for p in (0, 2, "big")}
    for a, b in itertools.combinations(pads, 2):
        assert any(x != y for x, y in zip(pads[a], pads[b])), "pads %s and %s give the same rows on every frame" % (a, b)
    for name, sets in list(rows.items()) + list(pads.items()):
        for f, s in enumerate(sets):
            assert any(r[0] == 0 for r in s), "%s: frame %d has no row on level 0" % (name, f)


# ----------------------------------------------------------------------------- gray_tail and the restatement agree on the windows

@pytest.mark.parametrize("fam", ["four", "five_cols"])
def test_the_oracle_has_the_windows_of_the_restatement(fam):
    """On maps of distinct values the window maxima of the oracle (its pooled map, resized back to the level: every window is
    reached) are the maxima over the restated windows, and the oracle pools windows_y * windows_x windows.  (The DISTINCT maxima are
    fewer than the windows on any map: the windows of an axis are nested prefixes and suffixes of it, and of two nested windows the
    outer one keeps the inner one's maximum unless its own lies outside -- which two crossing pairs cannot both have.)"""
    ext = kr.extents("G1")
    most = 0
    for l in (0, 3):
        h, w = ext[l]
        rh, rw = kr.regions(fam, ext)[l]
        t = kr.path(ext, kr.regions(fam, ext))[1][l]
        oh, wins_y, src_y = so._region_pool_geometry(h, rh)
        ow, wins_x, src_x = so._region_pool_geometry(w, rw)
        assert (oh, ow) == (t["wy"], t["wx"]) and wins_y == t["rows"] and wins_x == t["cols"]
        assert set(src_y.tolist()) == set(range(oh)) and set(src_x.tolist()) == set(range(ow))
        for seed in range(3):
            v = np.random.default_rng(seed).permutation(h * w).astype(np.float32).reshape(1, h, w, 1)
            want = {float(v[0, y0:y1, x0:x1, 0].max()) for y0, y1 in t["rows"] for x0, x1 in t["cols"]}
            got = set(np.unique(so.region_threshold(v, rh, rw)).tolist())
            assert got == want and len(got) <= t["wy"] * t["wx"]
            most = max(most, len(got))
    assert most > 1
