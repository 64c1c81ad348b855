"""silent_pyramid_bayer[_dev] and silent_bayer_to_rgb[_dev] (raw 8-bit Bayer mosaics, 3-channel plans) write ALL of their output and
NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between guards under two fills and at the weakest
alignment; the host form after a poisoned staging arena; the same call after other inputs) through the helpers of
tests/write_coverage.py, for a classic pyramid (one walk plan) and a crop layout (the union walk with its border pixels), on a window
at an odd row and an odd column of larger sensor images [2, H + 7, W + 26] and on every second byte of padded rows [2, H + 3, 2 W + 27].
And the buffers' other bytes do not reach a result: flipping every byte that is not a pixel of the view leaves every output bit
unchanged."""
import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
LAYOUTS = {"window": "bayer_gbrg", "second": "bayer_grbg"}
FAMILIES = ("ratio2_3", "reference_crop")
SIZES = (pg.FA, (148, 318))             # W % 4 == 0 and W % 4 == 2


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _rows(layout, hw):
    return (hw[0] + 7, hw[1] + 26) if layout == "window" else (hw[0] + 3, 2 * hw[1] + 27)


def _inputs(layout, hw, seed):
    def make():
        return [np.random.default_rng(seed).integers(0, 256, (2,) + _rows(layout, hw)).astype(np.uint8)]
    return make


def _mosaic(layout, hw, buffers):
    """The [2, H, W] view of the buffers (NumPy or torch; nothing copied)."""
    if layout == "window":
        return buffers[:, 3:3 + hw[0], 5:5 + hw[1]]
    return buffers[:, 1:1 + hw[0], 5:5 + 2 * hw[1]:2]


def _bayer_calls(layout, family, hw):
    def calls(rt, buffers):
        plan = wcc.plan_of(rt, ("bayer", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        m = _mosaic(layout, hw, buffers)
        return [lambda: (plan.run(m, rgb_frame_format=LAYOUTS[layout]),), lambda: (rt.bayer_to_rgb(m, hw, LAYOUTS[layout], "rgb"),)]
    return calls


def _parse(case):
    _, layout, family, size = case.id.split("-")
    return layout, family, tuple(int(v) for v in size.split("x"))


CASES = []
for _li, _layout in enumerate(LAYOUTS):
    for _fi, _family in enumerate(FAMILIES):
        for _hw in SIZES:
            _px = 2 * max(sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw)), _hw[0] * _hw[1])
            CASES.append(wcc.Case("bayer-%s-%s-%dx%d" % (_layout, _family, _hw[0], _hw[1]), _bayer_calls(_layout, _family, _hw),
                                  _inputs(_layout, _hw, 3100 + 10 * _li + _fi), _px * 3 * 4 + 4096, workspace=True))
IDS = [c.id for c in CASES]


def test_the_cases_take_the_walk_kernel(rt):
    for case in CASES:
        _, family, hw = _parse(case)
        plan = wcc.plan_of(rt, ("bayer", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        assert plan.walk_plans[0] >= 1, (case.id, plan.walk_plans)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bayer_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bayer_host_form_does_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bayer_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bytes_that_are_no_pixels_do_not_reach_a_result(rt, case):
    """Every byte of the buffers that is not a pixel of the view -- the sensor around the window, the bytes between the pixels, the
    padding of each row -- flipped (x ^ 0xFF): the pyramid and the converted frames keep every bit, _dev form and host form."""
    import torch
    layout, _, hw = _parse(case)
    buffers = np.array(case.inputs()[0])
    marks = np.zeros(buffers.shape, np.uint8)
    _mosaic(layout, hw, marks)[...] = 1
    mask = marks.astype(bool)
    assert 0 < mask.sum() == 2 * hw[0] * hw[1] < mask.size
    flipped = np.where(mask, buffers, buffers ^ 0xFF).astype(np.uint8)
    assert np.array_equal(flipped[mask], buffers[mask]) and np.all(flipped[~mask] != buffers[~mask])
    for place in (lambda a: torch.from_numpy(a).cuda(0), lambda a: a):
        a, b = case.calls(rt, place(buffers)), case.calls(rt, place(flipped))
        for fa, fb in zip(a, b):
            for ra, rb in zip(fa(), fb()):
                ra, rb = (r.data if type(r).__name__ == "PackedPyramid" else r for r in (ra, rb))
                ra, rb = (r.cpu().numpy() if hasattr(r, "cpu") else r for r in (ra, rb))
                assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), case.id
