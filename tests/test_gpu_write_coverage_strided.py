"""The strided-view entry points (silent_pyramid_view, silent_gray_pass_view, silent_gray_keypoints_view, host and _dev forms) write
ALL of their output and NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between guards under two fills and
at the weakest alignment; host forms after a poisoned staging arena; the same call after other inputs) through the helpers of
tests/write_coverage.py, on a region of a larger one-channel frame (odd pitch, odd offset) and on BGRA without its alpha byte, for a
streamable plan and a crop layout."""
import ctypes as C

import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage as wc
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
K = 4
STRIDED = dict(frame_dtype="uint8", frame_layout="strided")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _inputs(hw, seed):
    def make():
        rng = np.random.default_rng(seed)
        return [rng.integers(0, 256, (2, 163, 389)).astype(np.uint8), rng.integers(0, 256, (2, hw[0], hw[1], 4)).astype(np.uint8)]
    return make


def _views(hw, parent, bgra):
    """(frames, frame_channels): the region at (7, 5) of the larger frames, and the first three bytes of every BGRA pixel."""
    return (parent[:, 7:7 + hw[0], 5:5 + hw[1], None], 1), (bgra[..., :3], 3)


def _keypoints(rt, plan, frames, channels, selection):
    """silent_gray_keypoints_view[_dev] through the plan's operand, with the value map and (selection = 1) the peak-value map."""
    from pysilent_amd import _lib
    cs_k, bank = [np.ascontiguousarray(np.asarray(k, np.float64).astype(np.float32)) for k in wcc._gray_weights(K)]
    op = plan._frames(frames, frame_channels=channels, **STRIDED)
    n, px = op.n_frames, plan.frame_px
    (pyr, pp), (cso, cp), (endo, ep), (value, vp) = [op.empty(n * px * ch) for ch in (1, 1, K, 1)]
    peak, kp = op.empty(n * px) if selection else (None, None)
    idx, iptr = op.empty((n, px, 4), np.int64)
    counts, cptr = op.empty(n, np.int64)
    reg = (_lib.Extent * len(plan.extents))(*[_lib.Extent(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents])
    op.call(plan._entry("gray_keypoints", "uint8", channels, "strided"), plan.handle, op.ptr, n, C.c_void_p(cs_k.ctypes.data),
            C.c_void_p(bank.ctypes.data), K, 255.0, pp, cp, ep, 2, int(selection), 0.1, reg, vp, kp, iptr, px, cptr)
    return pyr, cso, endo, value, peak, wc.Rows(idx, counts)


def _view_calls(family, hw):
    def calls(rt, parent, bgra):
        plan = wcc.plan_of(rt, ("gray", family, hw), hw, 1, wcc.gray_family_levels(family, hw))
        cs_k, bank = wcc._gray_weights(K)
        (v1, c1), (v3, c3) = _views(hw, parent, bgra)
        assert not (v1.flags["C_CONTIGUOUS"] if isinstance(v1, np.ndarray) else v1.is_contiguous())
        return [lambda: (plan.run(v1, frame_channels=c1, **STRIDED),),
                lambda: (plan.run(v3, frame_channels=c3, **STRIDED),),
                lambda: plan.gray_pass(v1, cs_k, bank, frame_channels=c1, **STRIDED),
                lambda: plan.gray_pass(v3, cs_k, bank, storage="float16", frame_channels=c3, **STRIDED),
                lambda: _keypoints(rt, plan, v1, c1, True),
                lambda: _keypoints(rt, plan, v3, c3, False)]
    return calls


CASES = []
for _fi, _family in enumerate(("ratio2_3", "reference_crop")):
    for _hw in (pg.FA, pg.FB):
        _px = 2 * sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw))
        CASES.append(wcc.Case("view-%s-%dx%d-K%d" % (_family, _hw[0], _hw[1], K), _view_calls(_family, _hw), _inputs(_hw, 880 + _fi),
                              _px * ((2 + K) * 4 + 8 + 32) + 4096, workspace=True))
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_view_device_forms_write_all_and_only_their_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_view_host_forms_do_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_view_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)
