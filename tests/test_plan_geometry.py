"""CPU side of the plan-geometry cases (tests/plan_geometry.py): the three references agree bit for bit on every case, every
named mistake a planner or kernel could make fails the GPU file's own assertion on the case classes meant to catch it (and most
pass on the geometry classic_levels() / reference_levels() produce -- why the cases exist), a float32 evaluation in another order
meets that assertion, and the planner -- run on the host alone -- accepts every case and routes it where the ROUTES column says.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_geometry as pg
from conftest import ROOT

NAMES = sorted(pg.CASES)


def _frame(case, channels=3):
    return pg.frames_of(case["frame"], channels, 1)[0]


def _flat(levels):
    return np.concatenate([np.asarray(l).reshape(-1) for l in levels])


def _passes(got_flat, want_levels, levels, channels):
    """Does a pyramid pass the assertion tests/test_gpu_plan_geometry.py makes?"""
    import conftest
    try:
        pg.assert_levels_close(pg.split(got_flat, levels, channels), want_levels, "sensitivity")
    except AssertionError:
        return False
    finally:                         # an oracle-vs-oracle comparison has no place in the end-of-suite error summary
        conftest.WORST_BOUND.pop("sensitivity", None)
        conftest.WORST_REL.pop("sensitivity", None)
    return True


def test_the_cases_are_valid_and_cover_both_frames_and_every_residue():
    residues = {w: set() for w in (316, 317)}
    for name, case in pg.CASES.items():
        assert pg.is_valid(case["frame"], case["levels"]), name
        assert case["frame"] in (pg.FA, pg.FB)
        if "sub_window" in case["classes"]:
            units = [l for l in case["levels"] if pg.is_unit(l)]
            assert len(units) == 1 and all(l[:4] == units[0][:4] for l in case["levels"]), name
            residues[case["frame"][1]].add(units[0][1] % 4)
    assert residues[316] == {0, 1, 3} and residues[316] | residues[317] == {0, 1, 2, 3}
    assert set(pg.ROUTES) == set(pg.CASES)
    # the dead pairs are dead (other cases hold some by accident of their extents, 233 -> 29 for one)
    assert [pg.dead_axes(l) for l in pg.CASES["dead_316"]["levels"]] == [(False, False), (True, False), (False, True)]
    assert [pg.dead_axes(l) for l in pg.CASES["dead_317"]["levels"]] == [(True, True), (False, False), (True, False)]


@pytest.mark.parametrize("name", NAMES)
def test_the_three_references_agree_bit_for_bit(name):
    """c_oracle.zoom_level (what the GPU tests compare with), silent_oracle.spline5_zoom on the crop plus a clipped copy, and --
    where its own rounding of the extent lands on the level's zoom -- scipy.ndimage.zoom with one factor per axis."""
    case = pg.CASES[name]
    frame = _frame(case)
    want = pg.oracle_pyramid(frame, case["levels"])
    for a, b, lv in zip(want, pg.python_pyramid(frame, case["levels"]), case["levels"]):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (name, lv))
        if pg.scipy_applies(lv):
            np.testing.assert_array_equal(a, pg.scipy_level(frame, lv), err_msg="%s %s scipy" % (name, lv))
        assert not a[pg.zero_mask(lv)].any()
    # ... and evaluate() with no mistake switched on is that definition
    np.testing.assert_array_equal(pg.evaluate(frame, case["levels"]), _flat(want))
    assert sum(pg.scipy_applies(lv) for c in pg.CASES.values() for lv in c["levels"]) > 100


@pytest.mark.parametrize("name", [n for n in NAMES if "dead" in pg.CASES[n]["classes"] or n.startswith(("sub_br", "nested", "zoom_h"))])
def test_the_references_agree_on_nonfinite_pixels(name):
    """NaN / inf pixels inside every crop, a NaN under every dead row / column: scipy emits cval = 0 there WITHOUT reading a pixel,
    so the NaN stays out of the level -- and so say both oracles (their 0 * NaN used to let it in)."""
    case = pg.CASES[name]
    frame = pg.poisoned_inside(_frame(case), case["levels"])
    with np.errstate(invalid="ignore", over="ignore"):
        want = pg.oracle_pyramid(frame, case["levels"])
        for a, b, lv in zip(want, pg.python_pyramid(frame, case["levels"]), case["levels"]):
            assert np.array_equal(a, b, equal_nan=True), (name, lv)
            if pg.scipy_applies(lv):
                assert np.array_equal(a, pg.scipy_level(frame, lv), equal_nan=True), (name, lv)
            assert not np.nan_to_num(a[pg.zero_mask(lv)], nan=1.0).any()
    assert any(np.isnan(w).any() for w in want)


@pytest.mark.parametrize("mutant", sorted(pg.MUTANTS))
def test_every_mistake_fails_the_gpu_tests_assertion_on_its_classes(mutant):
    kw, classes = pg.MUTANTS[mutant]
    n = 0
    for name in NAMES:
        case = pg.CASES[name]
        if not case["classes"] & set(classes):
            continue
        for channels in (1, 3):
            frame = _frame(case, channels)
            want = pg.oracle_pyramid(frame, case["levels"])
            assert not _passes(pg.evaluate(frame, case["levels"], **kw), want, case["levels"], channels), (mutant, name, channels)
        n += 1
    assert n >= 2, (mutant, n)


# what the two generators let through (the frame is not square, so exchanging the two zoom extents is seen on both; the reference's
# crops have origins of their own and inner crop edges; this layout's canvases are never smaller than their zoom)
PASS_ON_CLASSIC = {"origin_ignored", "origin_swapped", "frame_edge_mirror", "canvas_not_clipped", "sorted_order", "second_unit_at_first"}
PASS_ON_REFERENCE = {"canvas_not_clipped", "sorted_order", "second_unit_at_first", "dead_row_kept"}


def test_most_mistakes_pass_on_the_geometry_the_generators_produce():
    """Why the cases exist.  (This classic pyramid holds a dead pair, 316 -> 40, as the whole-frame ones of tests/test_gpu_parity.py
    do; this reference layout holds none.)"""
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    seen = {}
    for tag, levels in (("classic", classic_levels(pg.FA, 2.0, 4)), ("reference", reference_levels(pg.FA, (80, 40), math.e ** .5))):
        assert len(levels) >= 3
        frame = pg.frames_of(pg.FA, 3, 1)[0]
        want = pg.oracle_pyramid(frame, levels)
        seen[tag] = {m for m, (kw, _) in pg.MUTANTS.items() if _passes(pg.evaluate(frame, levels, **kw), want, levels, 3)}
    assert seen["classic"] == PASS_ON_CLASSIC
    assert seen["reference"] == PASS_ON_REFERENCE
    # nothing but the extent exchange and the dead pair is seen on a classic pyramid, and the generators share three blind spots
    assert set(pg.MUTANTS) - seen["classic"] == {"zoom_swapped", "dead_row_kept"}
    assert seen["classic"] & seen["reference"] == {"canvas_not_clipped", "sorted_order", "second_unit_at_first"}


def _attainable(frame_hw, channels, levels, tag):
    frame = pg.frames_of(frame_hw, channels, 1)[0]
    want = pg.oracle_pyramid(frame, levels)
    pg.assert_levels_close(pg.float32_pyramid(frame, levels), want, "float32 plan geometry " + tag)


@pytest.mark.parametrize("name", NAMES)
def test_a_float32_evaluation_meets_the_gpu_tests_assertion(name):
    """The bound can be met: two separable float32 passes in torch, on frames of the GPU test's kind."""
    pytest.importorskip("torch")
    case = pg.CASES[name]
    for channels in (1, 3):
        _attainable(case["frame"], channels, case["levels"], "cases")


def test_a_float32_evaluation_meets_the_assertion_on_the_random_plans():
    pytest.importorskip("torch")
    for seed in pg.RANDOM_SEEDS:
        hw, channels, levels = pg.random_case(seed)
        assert pg.is_valid(hw, levels)
        _attainable(hw, channels, levels, "random")


def test_random_levels_mix_the_properties():
    stats = dict(units=0, two_units=0, no_unit=0, up=0, aniso=0, clip=0, grow=0, offset=0, unsorted=0, degenerate=0)
    for seed in pg.RANDOM_SEEDS:
        hw, channels, levels = pg.random_case(seed)
        assert pg.random_case(seed) == (hw, channels, levels)                  # a pure function of the seed
        n_unit = sum(pg.is_unit(l) for l in levels)
        stats["units"] += n_unit >= 1
        stats["two_units"] += n_unit >= 2
        stats["no_unit"] += n_unit == 0
        stats["up"] += any(l[4] > l[2] or l[5] > l[3] for l in levels)
        stats["aniso"] += any(abs(l[4] / l[2] - l[5] / l[3]) > 0.05 for l in levels)
        stats["clip"] += any(l[6] < l[4] or l[7] < l[5] for l in levels)
        stats["grow"] += any(l[6] > l[4] or l[7] > l[5] for l in levels)
        stats["offset"] += any(l[0] > 0 and l[1] > 0 and l[0] + l[2] < hw[0] and l[1] + l[3] < hw[1] for l in levels)
        r = [l[5] / l[3] for l in levels]
        stats["unsorted"] += r != sorted(r, reverse=True)
        stats["degenerate"] += any(min(l[2:6]) < 5 for l in levels)
    assert all(v >= 4 for v in stats.values()), stats


# ----------------------------------------------------------------------------- routes (host-only build, no GPU)

@pytest.fixture(scope="module")
def routes():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    from test_sanitizers import SAN_ENV
    lib = B.build_host_asan()
    rt_lib = B.asan_runtime()
    if rt_lib is None:
        pytest.skip("the ROCm LLVM has no shared asan runtime")
    env = dict(os.environ, LD_PRELOAD=rt_lib, SILENT_LIB_PATH=lib, **SAN_ENV)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plan_geometry_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    out = p.stdout
    assert p.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    line = [l for l in out.splitlines() if l.startswith("plan geometry routes: ")]
    assert len(line) == 1, out[-4000:]
    return json.loads(line[0].split(": ", 1)[1])


def test_every_valid_plan_is_created(routes):
    """SILENT_OK for every case at 1 and 3 channels and for every random plan: no refusal, no 'internal error'."""
    assert routes["refused"] == []
    assert len(routes["cases"]) == 2 * len(pg.CASES) and len(routes["random"]) == len(pg.RANDOM_SEEDS)


def test_the_planner_routes_every_case_as_recorded(routes):
    reached = {}
    for name in NAMES:
        levels = pg.CASES[name]["levels"]
        for k, channels in enumerate((1, 3)):
            streamable, walk = routes["cases"]["%s/%d" % (name, channels)]
            assert (streamable, tuple(walk)) == pg.ROUTES[name][k], (name, channels)
            if channels == 1:
                assert (pg.stream_layout(levels) is not None) == streamable, name      # the restated eligibility test holds
            else:
                assert not streamable
            for tag in pg.route_tags(levels, channels, streamable, tuple(walk)):
                reached.setdefault(tag, []).append("%s/%d" % (name, channels))
    for route in pg.REQUIRED_ROUTES:
        assert len(reached.get(route, [])) >= 2, (route, reached.get(route))
    for px in (36, 32, 28):
        assert any(pg.ROUTES[n][1][1][1] == px for n in NAMES), px
    for seed, (streamable, walk) in routes["random"].items():
        hw, channels, levels = pg.random_case(int(seed))
        if channels == 1:
            assert (pg.stream_layout(levels) is not None) == streamable, seed
