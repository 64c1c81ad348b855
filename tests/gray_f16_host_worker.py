"""Worker of tests/test_gray_float16_host.py: runs against the host-only build of the library (kernel launches compiled out,
device memory = host memory; pysilent_amd/csrc/silent_host_shim.h) -- silent_gray_pass_h's argument validation and status codes,
and the host code of the float16-storage pass (its staging through HostStage, every kernel family's launch path), no GPU."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pysilent_amd import _lib, _runtime as rt  # noqa: E402
from pysilent_amd import constant_convolutions as cc  # noqa: E402
from pysilent_amd.pipeline import default_constants  # noqa: E402
from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels  # noqa: E402

lib = _lib.load()
assert "hostonly" in _lib.LIB_PATH, "this worker must never run against the product library"
ctx = rt.get_context(0)
GRAY = default_constants("gray", 4)
H, W = 40, 57                    # (odd width: CS rows start on 2-byte boundaries)
levels = classic_levels((H, W), 2.0, 3)
frames = np.ascontiguousarray(np.random.default_rng(0).random((2, H, W, 1), dtype=np.float32) * 255.0)
cs_k = np.ascontiguousarray(GRAY["cs"], np.float32)


def call(plan_handle, K=4, n=2, frames_ptr=True, pyr_ptr=True, cs_ptr=True, end_ptr=True, px=None, dev=False, parts=3):
    """silent_gray_pass_h[_dev] with buffers of the right size (host memory is device memory in this build) -> status."""
    px = px or sum(l[6] * l[7] for l in levels)
    end_k = np.ascontiguousarray(cc.end_bank(K if K in (3, 4, 8) else 4), np.float32)
    pyr = np.zeros(n * px, np.float32)
    cs = np.zeros(n * px, np.uint16)
    end = np.zeros(n * px * max(K, 1), np.uint16)
    args = [ctx.handle, plan_handle, frames.ctypes.data if frames_ptr else None, n, cs_k.ctypes.data, end_k.ctypes.data, K, 255.0,
            pyr.ctypes.data if pyr_ptr else None, _lib.half_ptr(cs.ctypes.data if cs_ptr else None),
            _lib.half_ptr(end.ctypes.data if end_ptr else None)]
    if dev:
        return lib.silent_gray_pass_h_dev(*(args + [parts, None]))
    return lib.silent_gray_pass_h(*args)


plan = rt.PyramidPlan(H, W, 1, levels, 0)
plan64 = rt.PyramidPlan(H, W, 1, levels, 0, accumulation="float64")
plan3 = rt.PyramidPlan(H, W, 3, levels, 0)
for dev in (False, True):
    assert call(plan.handle, dev=dev) == _lib.SILENT_OK
    assert call(plan.handle, cs_ptr=False, dev=dev) == _lib.SILENT_OK          # cs_out = NULL
    assert call(plan.handle, end_ptr=False, dev=dev) == _lib.SILENT_OK         # end_out = NULL
    assert call(plan.handle, cs_ptr=False, end_ptr=False, dev=dev) == _lib.SILENT_E_INVALID
    assert call(None, dev=dev) == _lib.SILENT_E_INVALID                        # NULL plan
    assert call(plan.handle, frames_ptr=False, dev=dev) == _lib.SILENT_E_INVALID
    assert call(plan.handle, pyr_ptr=False, dev=dev) == _lib.SILENT_E_INVALID
    assert call(plan.handle, n=0, dev=dev) == _lib.SILENT_E_INVALID
    assert call(plan64.handle, dev=dev) == _lib.SILENT_E_UNSUPPORTED           # SILENT_PLAN_ACCUM_F64 plan
    assert call(plan3.handle, dev=dev) == _lib.SILENT_E_UNSUPPORTED            # 3-channel plan
    for K in (0, 1, 2, 5, 7, 9, -1):
        assert call(plan.handle, K=K, dev=dev) == _lib.SILENT_E_UNSUPPORTED, K  # bad n_orient
    for K in (3, 4, 8):
        assert call(plan.handle, K=K, dev=dev) == _lib.SILENT_OK
assert call(plan.handle, dev=True, parts=0) == _lib.SILENT_E_INVALID
assert call(plan.handle, dev=True, parts=1) == _lib.SILENT_OK and call(plan.handle, dev=True, parts=2) == _lib.SILENT_OK
assert lib.silent_gray_pass_h(None, plan.handle, None, 1, None, None, 4, 255.0, None, None, None) == _lib.SILENT_E_INVALID   # NULL context
assert "float16" in _lib.last_error(ctx.handle) or _lib.last_error(ctx.handle)
for p in (plan, plan64, plan3):
    p.close()

# the Python layer over it: every kernel family's host path (stream layouts 0 and 1, one level, the crop layout's unit-fused path)
f2 = np.ascontiguousarray(np.random.default_rng(1).random((2, 40, 56, 1), dtype=np.float32) * 255.0)
for lv in (classic_levels((40, 56), 2.0, 3), classic_levels((40, 56), 2.0 ** .5, 6), classic_levels((40, 56), 2.0, 1),
           reference_levels((40, 56), (20, 12), np.e ** .5)):
    plan = rt.PyramidPlan(40, 56, 1, lv, 0)
    for K in (3, 4, 8):
        pyr, cs, end = plan.gray_pass(f2, GRAY["cs"], cc.end_bank(K).astype(np.float32), storage="float16")
        assert pyr.data.dtype == np.float32 and cs.data.dtype == np.float16 and end.data.dtype == np.float16
        assert cs.dtype == np.float16 and end.channels == K and end.level(0).shape == (2, lv[0][6], lv[0][7], K)
        assert end.data.nbytes == 2 * 2 * plan.frame_px * K
    plan.close()
plan64 = rt.PyramidPlan(40, 56, 1, classic_levels((40, 56), 2.0, 3), 0, accumulation="float64")
for kw in (dict(storage="bfloat16"), dict(storage=None), dict(storage="float16")):   # (the last one: a float64 plan)
    try:
        plan64.gray_pass(f2, GRAY["cs"], GRAY["end"], **kw)
    except ValueError:
        continue
    raise AssertionError("gray_pass(%r) on a float64 plan was accepted" % (kw,))
plan64.close()
print("gray float16 host worker ok")
