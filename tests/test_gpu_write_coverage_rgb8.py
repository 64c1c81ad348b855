"""silent_pyramid_rgb8 and silent_pyramid_rgb8_dev (packed interleaved uint8 colour frames, 3-channel plans) write ALL of their output
and NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between guards under two fills and at the weakest
alignment; the host form after a poisoned staging arena; the same call after other inputs) through the helpers of
tests/write_coverage.py, for a classic pyramid (one walk plan) and a crop layout (the union walk with its border pixels), on frames
pg.FA (W % 4 == 0: the dword loader) and pg.FB (3 * W % 4 == 3: the one-byte loader)."""
import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
RGB8 = dict(rgb_frame_dtype="uint8")
FAMILIES = ("ratio2_3", "reference_crop")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _inputs(hw, seed):
    return lambda: [np.random.default_rng(seed).integers(0, 256, (2, hw[0], hw[1], 3)).astype(np.uint8)]


def _rgb8_calls(family, hw):
    def calls(rt, u8):
        plan = wcc.plan_of(rt, ("rgb8", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        return [lambda: (plan.run(u8, **RGB8),)]
    return calls


CASES = []
for _fi, _family in enumerate(FAMILIES):
    for _hw in (pg.FA, pg.FB):
        _px = 2 * sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw))
        CASES.append(wcc.Case("rgb8-%s-%dx%d" % (_family, _hw[0], _hw[1]), _rgb8_calls(_family, _hw), _inputs(_hw, 2400 + _fi),
                              _px * 3 * 4 + 4096, workspace=True))
IDS = [c.id for c in CASES]


def test_the_cases_take_the_walk_kernel(rt):
    """The routes the cases are meant to reach: one walk plan for the classic pyramid, a unit plan + the union plan for the crops."""
    for case in CASES:
        family, hw = case.id.split("-")[1], tuple(int(v) for v in case.id.split("-")[2].split("x"))
        plan = wcc.plan_of(rt, ("rgb8", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        assert plan.walk_plans[0] >= 1, (case.id, plan.walk_plans)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rgb8_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rgb8_host_form_does_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rgb8_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)
