"""The uint16 entry points (silent_pyramid_u16, silent_gray_pass_u16, silent_gray_keypoints_u16 and their *_view16 twins, host and
_dev forms: twelve) write ALL of their output and NOTHING else: the three checks of tests/test_gpu_write_coverage.py (results between
guards under two fills and at the weakest alignment; host forms after a poisoned staging arena; the same call after other inputs)
through the helpers of tests/write_coverage.py, on a packed batch and on a window at (7, 5) of larger frames (odd pitch in elements,
odd offset), for a streamable plan and a crop layout."""
import ctypes as C

import numpy as np
import pytest

import plan_geometry as pg
import test_gpu_write_coverage as tg
import write_coverage as wc
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu
K = 4
FULL = 65535.0
PACKED = dict(frame_dtype="uint16")
STRIDED = dict(frame_dtype="uint16", frame_layout="strided")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _inputs(hw, seed):
    def make():
        rng = np.random.default_rng(seed)
        return [rng.integers(0, 65536, (2, hw[0], hw[1], 1)).astype(np.uint16), rng.integers(0, 65536, (2, 163, 389)).astype(np.uint16)]
    return make


def _u16(x):
    """An input as uint16 (the helpers' "other values" of a non-uint8 input are float32 noise in 0 .. 64: exact as uint16)."""
    if isinstance(x, np.ndarray):
        return x if x.dtype == np.uint16 else x.astype(np.uint16)
    import torch
    return x if x.dtype == torch.uint16 else x.to(torch.uint16)


def _keypoints(rt, plan, frames, kind, selection):
    """silent_gray_keypoints_u16 / _view16 [_dev] through the plan's operand, with the value map and (selection = 1) the peak-value map."""
    from pysilent_amd import _lib
    cs_k, bank = [np.ascontiguousarray(np.asarray(k, np.float64).astype(np.float32)) for k in wcc._gray_weights(K)]
    op = plan._frames(frames, **kind)
    n, px = op.n_frames, plan.frame_px
    (pyr, pp), (cso, cp), (endo, ep), (value, vp) = [op.empty(n * px * ch) for ch in (1, 1, K, 1)]
    peak, kp = op.empty(n * px) if selection else (None, None)
    idx, iptr = op.empty((n, px, 4), np.int64)
    counts, cptr = op.empty(n, np.int64)
    reg = (_lib.Extent * len(plan.extents))(*[_lib.Extent(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents])
    op.call(plan._entry("gray_keypoints", "uint16", 1, kind.get("frame_layout", "packed")), plan.handle, op.ptr, n, C.c_void_p(cs_k.ctypes.data),
            C.c_void_p(bank.ctypes.data), K, FULL, pp, cp, ep, 2, int(selection), 0.1, reg, vp, kp, iptr, px, cptr)
    return pyr, cso, endo, value, peak, wc.Rows(idx, counts)


def _u16_calls(family, hw):
    def calls(rt, packed, parent):
        plan = wcc.plan_of(rt, ("gray", family, hw), hw, 1, wcc.gray_family_levels(family, hw))
        cs_k, bank = wcc._gray_weights(K)
        packed, parent = _u16(packed), _u16(parent)
        view = parent[:, 7:7 + hw[0], 5:5 + hw[1]]
        assert not (view.flags["C_CONTIGUOUS"] if isinstance(view, np.ndarray) else view.is_contiguous())
        return [lambda: (plan.run(packed, **PACKED),),
                lambda: plan.gray_pass(packed, cs_k, bank, FULL, **PACKED),
                lambda: plan.gray_pass(packed, cs_k, bank, FULL, storage="float16", **PACKED),
                lambda: _keypoints(rt, plan, packed, PACKED, True),
                lambda: (plan.run(view, **STRIDED),),
                lambda: plan.gray_pass(view, cs_k, bank, FULL, **STRIDED),
                lambda: plan.gray_pass(view, cs_k, bank, FULL, storage="float16", **STRIDED),
                lambda: _keypoints(rt, plan, view, STRIDED, False)]
    return calls


CASES = []
for _fi, _family in enumerate(("ratio2_3", "reference_crop")):
    for _hw in (pg.FA, pg.FB):
        _px = 2 * sum(l[6] * l[7] for l in wcc.gray_family_levels(_family, _hw))
        CASES.append(wcc.Case("u16-%s-%dx%d-K%d" % (_family, _hw[0], _hw[1], K), _u16_calls(_family, _hw), _inputs(_hw, 1680 + _fi),
                              _px * ((2 + K) * 4 + 8 + 32) + 4096, workspace=True))
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_u16_device_forms_write_all_and_only_their_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_u16_host_forms_do_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_u16_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)
