"""silent_pyramid_yuv16[_dev] and silent_yuv16_to_rgb[_dev] (planar, semi-planar and packed 16-bit YUV, 3-channel plans) write ALL of
their output and NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between guards under two fills and at the
weakest alignment; the host form after a poisoned staging arena; the same call after other inputs) through the helpers of
tests/write_coverage.py, for a classic pyramid (one walk plan) and a crop layout (the union walk with its border pixels), on I010
surfaces [2, H * 3 / 2 + 2, W + 26] elements (the chroma planes behind the luma rows at half the pitch) and on Y210 surfaces
[2, H + 3, 2 W + 27].  And the surfaces' other elements do not reach a result: flipping every element that is not a pixel's Y, U or V
leaves every output bit unchanged."""
import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
LAYOUTS = {"i010": "yuv420p10", "y210": "yuv422p10msb"}
FAMILIES = ("ratio2_3", "reference_crop")
SIZES = (pg.FA, (148, 318))             # W % 4 == 0 and W % 4 == 2


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _rows(layout, hw):
    return (hw[0] * 3 // 2 + 2, hw[1] + 26) if layout == "i010" else (hw[0] + 3, 2 * hw[1] + 27)


def _inputs(layout, hw, seed):
    def make():
        return [np.random.default_rng(seed).integers(0, 1 << 16, (2,) + _rows(layout, hw)).astype(np.uint16)]
    return make


def _u16(x):
    """An input as uint16 (the helpers' "other values" of a non-uint8 input are float32 noise in 0 .. 64: exact as uint16)."""
    if isinstance(x, np.ndarray):
        return x if x.dtype == np.uint16 else x.astype(np.uint16)
    import torch
    return x if x.dtype == torch.uint16 else x.to(torch.uint16)


def _planes(layout, hw, surfaces):
    from pysilent_amd.util.zoom import yuv16_planes
    return yuv16_planes(_u16(surfaces), hw[0], hw[1], layout)


def _yuv16_calls(layout, family, hw):
    def calls(rt, surfaces):
        plan = wcc.plan_of(rt, ("yuv16", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        planes = _planes(layout, hw, surfaces)
        return [lambda: (plan.run(planes, rgb_frame_format=LAYOUTS[layout]),),
                lambda: (rt.yuv16_to_rgb(planes, hw, LAYOUTS[layout], "bt2020", "full", "rgb"),)]
    return calls


def _parse(case):
    _, layout, family, size = case.id.split("-")
    return layout, family, tuple(int(v) for v in size.split("x"))


CASES = []
for _li, _layout in enumerate(LAYOUTS):
    for _fi, _family in enumerate(FAMILIES):
        for _hw in SIZES:
            _px = 2 * max(sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw)), _hw[0] * _hw[1])
            CASES.append(wcc.Case("yuv16-%s-%s-%dx%d" % (_layout, _family, _hw[0], _hw[1]), _yuv16_calls(_layout, _family, _hw),
                                  _inputs(_layout, _hw, 3100 + 10 * _li + _fi), _px * 3 * 4 + 4096, workspace=True))
IDS = [c.id for c in CASES]


def test_the_cases_take_the_walk_kernel(rt):
    for case in CASES:
        _, family, hw = _parse(case)
        plan = wcc.plan_of(rt, ("yuv16", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        assert plan.walk_plans[0] >= 1, (case.id, plan.walk_plans)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_yuv16_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_yuv16_host_form_does_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_yuv16_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_elements_that_are_no_pixels_do_not_reach_a_result(rt, case):
    """Every element of the surfaces that is not a pixel's Y, U or V -- the padding of each row, the rows behind the planes -- flipped
    (x ^ 0xFFFF): the pyramid and the converted frames keep every bit, _dev form and host form."""
    import torch
    layout, _, hw = _parse(case)
    surfaces = np.array(case.inputs()[0])
    marks = np.zeros(surfaces.shape, np.uint16)
    for p in _planes(layout, hw, marks):
        p[...] = 1
    mask = marks.astype(bool)
    per_pixel = {"i010": 1.5, "y210": 2.0}[layout]
    assert 0 < mask.sum() == int(2 * hw[0] * hw[1] * per_pixel) < mask.size
    flipped = np.where(mask, surfaces, surfaces ^ 0xFFFF).astype(np.uint16)
    assert np.array_equal(flipped[mask], surfaces[mask]) and np.all(flipped[~mask] != surfaces[~mask])
    for place in (lambda a: torch.from_numpy(a).cuda(0), lambda a: a):
        a, b = case.calls(rt, place(surfaces)), case.calls(rt, place(flipped))
        for fa, fb in zip(a, b):
            for ra, rb in zip(fa(), fb()):
                ra, rb = (r.data if type(r).__name__ == "PackedPyramid" else r for r in (ra, rb))
                ra, rb = (r.cpu().numpy() if hasattr(r, "cpu") else r for r in (ra, rb))
                assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), case.id
