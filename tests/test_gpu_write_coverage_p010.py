"""silent_pyramid_p010[_dev] and silent_p010_to_rgb[_dev] (P010 / P012 / P016 decoder surfaces, 3-channel plans) write ALL of their
output and NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between guards under two fills and at the
weakest alignment; the host form after a poisoned staging arena; the same call after other inputs) through the helpers of
tests/write_coverage.py, for a classic pyramid (one walk plan) and a crop layout (the union walk with its border pixels), on uint16
surfaces [2, H * 3 / 2 + 5, W + 27] whose chroma rows start 5 rows below the luma.  And nothing but the codes reaches a result:
flipping every element that is not a pixel's Y or part of a pixel's (U, V) pair, or the low 16 - depth bits of every element that is,
leaves every output bit unchanged."""
import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
P010 = dict(rgb_frame_format="p010")
FAMILIES = ("ratio2_3", "reference_crop")
SIZES = (pg.FA, (148, 318))             # W % 4 == 0 and W % 4 == 2


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _rows(hw):
    return hw[0] * 3 // 2 + 5, hw[1] + 27


def _inputs(hw, seed):
    def make():
        return [np.random.default_rng(seed).integers(0, 65536, (2,) + _rows(hw)).astype(np.uint16)]      # (random low bits)
    return make


def _u16(x):
    """An input as uint16 (the helpers' "other values" of a non-uint8 input are float32 noise in 0 .. 64: exact as uint16)."""
    if isinstance(x, np.ndarray):
        return x if x.dtype == np.uint16 else x.astype(np.uint16)
    import torch
    return x if x.dtype == torch.uint16 else x.to(torch.uint16)


def _planes(hw, surfaces):
    from pysilent_amd.util.zoom import p010_planes
    return p010_planes(_u16(surfaces), hw[0], hw[1], chroma_row=hw[0] + 5)


def _p010_calls(family, hw):
    def calls(rt, surfaces):
        plan = wcc.plan_of(rt, ("p010", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        planes = _planes(hw, surfaces)
        return [lambda: (plan.run(planes, **P010),), lambda: (rt.p010_to_rgb(planes, hw, 10, "bt2020", "full", "rgb"),)]
    return calls


CASES = []
for _fi, _family in enumerate(FAMILIES):
    for _hw in SIZES:
        _px = 2 * max(sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw)), _hw[0] * _hw[1])
        CASES.append(wcc.Case("p010-%s-%dx%d" % (_family, _hw[0], _hw[1]), _p010_calls(_family, _hw), _inputs(_hw, 2900 + _fi),
                              _px * 3 * 4 + 4096, workspace=True))
IDS = [c.id for c in CASES]


def test_the_cases_take_the_walk_kernel(rt):
    for case in CASES:
        family, hw = case.id.split("-")[1], tuple(int(v) for v in case.id.split("-")[2].split("x"))
        plan = wcc.plan_of(rt, ("p010", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
        assert plan.walk_plans[0] >= 1, (case.id, plan.walk_plans)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_p010_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_p010_host_form_does_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_p010_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)


def _same_results(rt, case, a, b):
    import torch
    for place in (lambda x: torch.from_numpy(x).cuda(0), lambda x: x):
        ca, cb = case.calls(rt, place(a)), case.calls(rt, place(b))
        for fa, fb in zip(ca, cb):
            for ra, rb in zip(fa(), fb()):
                ra, rb = (r.data if type(r).__name__ == "PackedPyramid" else r for r in (ra, rb))
                ra, rb = (r.cpu().numpy() if hasattr(r, "cpu") else r for r in (ra, rb))
                assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), case.id


def _pixel_mask(hw, shape):
    m16 = np.zeros(shape, np.uint16)
    for p in _planes(hw, m16):
        p[...] = 1
    return m16.astype(bool)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_elements_that_are_no_pixels_do_not_reach_a_result(rt, case):
    """Every element of the surfaces that is not a pixel's Y or part of a pixel's (U, V) pair -- the padding of each row, the five rows
    between the planes -- flipped (x ^ 0xFFFF): the pyramid and the converted frames keep every bit, _dev form and host form."""
    hw = tuple(int(v) for v in case.id.split("-")[2].split("x"))
    surfaces = np.array(case.inputs()[0])
    mask = _pixel_mask(hw, surfaces.shape)
    assert 0 < mask.sum() == 2 * hw[0] * hw[1] * 3 // 2 < mask.size
    flipped = np.where(mask, surfaces, surfaces ^ 0xFFFF).astype(np.uint16)
    assert np.array_equal(flipped[mask], surfaces[mask]) and np.all(flipped[~mask] != surfaces[~mask])
    _same_results(rt, case, surfaces, flipped)


@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_the_low_bits_do_not_reach_a_result(rt, case):
    """The low 6 bits of every pixel element flipped (depth 10): every output bit stays; the lowest bit of the CODE flipped: it does not."""
    hw = tuple(int(v) for v in case.id.split("-")[2].split("x"))
    surfaces = np.array(case.inputs()[0])
    mask = _pixel_mask(hw, surfaces.shape)
    assert np.any(surfaces[mask] & 0x3F)
    _same_results(rt, case, surfaces, np.where(mask, surfaces ^ 0x3F, surfaces).astype(np.uint16))
    with pytest.raises(AssertionError):
        _same_results(rt, case, surfaces, np.where(mask, surfaces ^ 0x40, surfaces).astype(np.uint16))
