"""Worker of tests/test_plan_geometry.py: runs INSIDE a python started with the sanitizer runtime preloaded and SILENT_LIB_PATH =
the host-only build of the library (as tests/sanitizer_worker.py does; no GPU).  Creates the plan of every case of
tests/plan_geometry.py for 1 and 3 channels and of every random case, drives it once through silent_pyramid and silent_gray_pass
(launches compiled out: the host code of the launch paths), and prints what the planner decided as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import plan_geometry as pg  # noqa: E402
from pysilent_amd import _lib, _runtime as rt  # noqa: E402
from pysilent_amd.pipeline import default_constants  # noqa: E402

_lib.load()
assert "hostonly" in _lib.LIB_PATH, "this worker must never run against the product library"
GRAY = default_constants("gray", 4)


def drive(frame_hw, channels, levels):
    plan = rt.PyramidPlan(frame_hw[0], frame_hw[1], channels, levels, 0)      # (raises on any status but SILENT_OK)
    route = [bool(plan.streamable), list(plan.walk_plans)]
    frames = np.zeros((2, frame_hw[0], frame_hw[1], channels), np.float32)
    plan.run(frames)
    if channels == 1:
        plan.gray_pass(frames, GRAY["cs"], GRAY["end"])
    plan.close()
    return route


out = {"cases": {}, "random": {}, "refused": []}
for name, case in pg.CASES.items():
    for c in (1, 3):
        try:
            out["cases"]["%s/%d" % (name, c)] = drive(case["frame"], c, case["levels"])
        except Exception as e:                                                   # noqa: BLE001
            out["refused"].append("%s/%d: %s" % (name, c, e))
for seed in pg.RANDOM_SEEDS:
    hw, c, levels = pg.random_case(seed)
    try:
        out["random"][str(seed)] = drive(hw, c, levels)
    except Exception as e:                                                       # noqa: BLE001
        out["refused"].append("random %d: %s" % (seed, e))
print("plan geometry routes: " + json.dumps(out))
