"""silent_pyramid_rgb8_view and silent_pyramid_rgb8_view_dev (strided uint8 colour views, 3-channel plans) write ALL of their output
and NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between guards under two fills and at the weakest
alignment; the host form after a poisoned staging arena; the same call after other inputs) through the helpers of
tests/write_coverage.py, for a classic pyramid (one walk plan) and a crop layout (the union walk with its border pixels), on frames
pg.FA and pg.FB, each as a region at (7, 5) of larger frames (odd pitch, odd offset) and as BGRA without its fourth byte."""
import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
STRIDED = dict(rgb_frame_dtype="uint8", rgb_frame_layout="strided")
FAMILIES = ("ratio2_3", "reference_crop")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _inputs(hw, seed):
    def make():
        rng = np.random.default_rng(seed)
        return [rng.integers(0, 256, (2, hw[0] + 20, hw[1] + 13, 3)).astype(np.uint8), rng.integers(0, 256, (2, hw[0], hw[1], 4)).astype(np.uint8)]
    return make


def _views(hw, parent, bgra):
    return parent[:, 7:7 + hw[0], 5:5 + hw[1]], bgra[..., :3]


def _view_calls(family, hw):
    def calls(rt, parent, bgra):
        plan = wcc.plan_of(rt, ("rgb8", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        region, bgr = _views(hw, parent, bgra)
        for v in (region, bgr):
            assert tuple(v.shape) == (2, hw[0], hw[1], 3) and not (v.flags["C_CONTIGUOUS"] if isinstance(v, np.ndarray) else v.is_contiguous())
        return [lambda: (plan.run(region, **STRIDED),), lambda: (plan.run(bgr, **STRIDED),)]
    return calls


CASES = []
for _fi, _family in enumerate(FAMILIES):
    for _hw in (pg.FA, pg.FB):
        _px = 2 * sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw))
        CASES.append(wcc.Case("rgb8view-%s-%dx%d" % (_family, _hw[0], _hw[1]), _view_calls(_family, _hw), _inputs(_hw, 2600 + _fi),
                              _px * 3 * 4 + 4096, workspace=True))
IDS = [c.id for c in CASES]


def test_the_cases_take_the_walk_kernel(rt):
    """The routes the cases are meant to reach: one walk plan for the classic pyramid, a unit plan + the union plan for the crops."""
    for case in CASES:
        family, hw = case.id.split("-")[1], tuple(int(v) for v in case.id.split("-")[2].split("x"))
        plan = wcc.plan_of(rt, ("rgb8", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        assert plan.walk_plans[0] >= 1, (case.id, plan.walk_plans)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rgb8_view_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rgb8_view_host_form_does_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rgb8_view_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)
