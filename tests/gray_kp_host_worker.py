"""Worker of tests/test_gray_keypoints_host.py: runs against the host-only build of the library (kernel launches compiled out,
device memory = host memory; pysilent_amd/csrc/silent_host_shim.h) -- silent_gray_keypoints' validation and host code, no GPU."""
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
frames = np.random.default_rng(0).random((2, 40, 56, 1), dtype=np.float32) * 255.0


def raises(fn, what):
    try:
        fn()
    except ValueError:
        return
    raise AssertionError("%s was accepted" % what)


for levels in (classic_levels((40, 56), 2.0, 3), reference_levels((40, 56), (20, 12), np.e ** .5)):
    plan = rt.PyramidPlan(40, 56, 1, levels, 0)
    for K in (3, 4, 8):
        for selection in (True, False):
            out = plan.gray_keypoints(frames, GRAY["cs"], cc.end_bank(K).astype(np.float32), pad=2, selection=selection)
            assert out[3].shape == (2, plan.frame_px, 4) and out[4].shape == (2,)
    end5 = np.zeros((3, 3, 1, 5), np.float32)
    raises(lambda: plan.gray_keypoints(frames, GRAY["cs"], end5), "n_orient = 5")
    raises(lambda: plan.gray_keypoints(frames, GRAY["cs"], GRAY["end"], pad=-1), "pad < 0")
    raises(lambda: plan.gray_keypoints(frames, GRAY["cs"], GRAY["end"], regions=[(4, 4)]), "one region for several levels")
    raises(lambda: plan.gray_keypoints(frames, GRAY["cs"], GRAY["end"], selection=2), "selection = 2")
    # NULL idx with a nonzero cap, and a peak-value map without selection: straight through the C ABI
    n = len(plan.extents)
    reg = (_lib.Extent * n)(*[_lib.Extent(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents])
    px = plan.frame_px * 2
    pyr, cs, end = np.zeros(px, np.float32), np.zeros(px, np.float32), np.zeros(px * 4, np.float32)
    counts, pv = np.zeros(2, np.int64), np.zeros(px, np.float32)
    f = frames.ctypes.data
    args = (ctx.handle, plan.handle, f, 2, GRAY["cs"].ctypes.data, GRAY["end"].ctypes.data, 4, 255.0, pyr.ctypes.data, cs.ctypes.data,
            end.ctypes.data, 2)
    raises(lambda: ctx.check(lib.silent_gray_keypoints(*args, 1, 0.1, reg, None, None, None, 16, counts.ctypes.data)), "NULL idx, cap 16")
    raises(lambda: ctx.check(lib.silent_gray_keypoints(*args, 0, 0.1, reg, None, pv.ctypes.data, None, 0, counts.ctypes.data)),
           "a peak-value map without selection")
    raises(lambda: ctx.check(lib.silent_gray_keypoints(*args, 1, 0.1, None, None, None, None, 0, counts.ctypes.data)), "NULL regions")
    ctx.check(lib.silent_gray_keypoints(*args, 1, 0.1, reg, None, None, None, 0, counts.ctypes.data))     # cap 0, no idx: fine
    plan.close()
# the selection entry points take 4 and 8 channels now, and still refuse 2
x = rt.PackedPyramid(np.random.default_rng(1).random(2 * 300 * 8, dtype=np.float32), [(10, 20), (10, 10)], 8, 2)
rt.select_peaks(x)
x2 = rt.PackedPyramid(np.random.default_rng(1).random(2 * 300 * 2, dtype=np.float32), [(10, 20), (10, 10)], 2, 2)
raises(lambda: rt.select_peaks(x2), "2 channels")
print("gray keypoints host worker ok")
