"""Worker of tests/test_gray_float64_host.py: runs against the host-only build of the library (kernel launches compiled out,
device memory = host memory; pysilent_amd/csrc/silent_host_shim.h) -- silent_pyramid_plan_create_ex's validation, the flags
round trip and the host code of float64 plans (their tables and launches), no GPU."""
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


def create(h, w, channels, levels, flags):
    arr = (_lib.PyrLevel * len(levels))(*[_lib.PyrLevel(*l) for l in levels])
    handle = C.c_void_p()
    rc = lib.silent_pyramid_plan_create_ex(ctx.handle, h, w, channels, arr, len(levels), flags, C.byref(handle))
    return rc, handle


def flags_of(handle):
    f = C.c_uint(12345)
    rc = lib.silent_pyramid_plan_flags(handle, C.byref(f))
    assert rc == _lib.SILENT_OK, rc
    return f.value


levels = classic_levels((40, 56), 2.0, 3)
# unknown flag bits: invalid, for 1 and 3 channels, alone or beside the known bit
for flags in (2, 3, 0x80000000, 0xffffffff):
    for ch in (1, 3):
        rc, h = create(40, 56, ch, levels, flags)
        assert rc == _lib.SILENT_E_INVALID and not h.value, (flags, ch, rc)
# float64 accumulation of an RGB plan: unsupported
rc, h = create(40, 56, 3, levels, _lib.PLAN_ACCUM_F64)
assert rc == _lib.SILENT_E_UNSUPPORTED and not h.value, rc
# the flags round-trip; silent_pyramid_plan_create is create_ex with 0
for ch, flags in ((1, 0), (1, _lib.PLAN_ACCUM_F64), (3, 0)):
    rc, h = create(40, 56, ch, levels, flags)
    assert rc == _lib.SILENT_OK, rc
    assert flags_of(h) == flags
    lib.silent_pyramid_plan_destroy(h)
arr = (_lib.PyrLevel * len(levels))(*[_lib.PyrLevel(*l) for l in levels])
h = C.c_void_p()
assert lib.silent_pyramid_plan_create(ctx.handle, 40, 56, 1, arr, len(levels), C.byref(h)) == _lib.SILENT_OK
assert flags_of(h) == 0
f = C.c_uint(0)
assert lib.silent_pyramid_plan_flags(None, C.byref(f)) == _lib.SILENT_E_INVALID
assert lib.silent_pyramid_plan_flags(h, None) == _lib.SILENT_E_INVALID
lib.silent_pyramid_plan_destroy(h)

# the host side of float64 plans: stream tables of every slot layout, the fallback, crop layouts; every entry point that honours it
frames = np.random.default_rng(0).random((2, 40, 56, 1), dtype=np.float32) * 255.0
for lv in (classic_levels((40, 56), 2.0, 3), classic_levels((40, 56), 2.0 ** .5, 6), classic_levels((40, 56), 2.0, 1),
           reference_levels((40, 56), (20, 12), np.e ** .5)):
    for acc in ("float32", "float64"):
        plan = rt.PyramidPlan(40, 56, 1, lv, 0, accumulation=acc)
        assert plan.accumulation == acc and plan.flags == (_lib.PLAN_ACCUM_F64 if acc == "float64" else 0)
        plan.run(frames)
        for K in (3, 4, 8):
            plan.gray_pass(frames, GRAY["cs"], cc.end_bank(K).astype(np.float32))
            out = plan.gray_keypoints(frames, GRAY["cs"], cc.end_bank(K).astype(np.float32), pad=2, selection=True)
            assert out[3].shape == (2, plan.frame_px, 4)
        plan.close()
for bad in ("float16", "double", None, 64):
    try:
        rt.PyramidPlan(40, 56, 1, levels, 0, accumulation=bad)
    except ValueError:
        continue
    raise AssertionError("accumulation=%r was accepted" % (bad,))
print("gray float64 host worker ok")
