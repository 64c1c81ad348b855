"""Float64 accumulation of the gray pass without a GPU: the ABI, argument validation (the library's host side built without a GPU
behind it, as tests/test_sanitizers.py builds it), and the premise the GPU tests rest on -- a separable float64 spline stored as
float32 is within 1 ulp of the oracle's 2-D float64 sum, and differs from it on a tiny share of the elements."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_float64_plan_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    for name in ("silent_pyramid_plan_create_ex", "silent_pyramid_plan_flags"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 5 and _lib.PLAN_ACCUM_F64 == 1
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    assert "#define SILENT_ABI_VERSION 5" in src and "#define SILENT_PLAN_ACCUM_F64 1u" in src


def test_library_exports_the_float64_plan_symbols():
    import ctypes
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "silent_pyramid_plan_create_ex") and hasattr(lib, "silent_pyramid_plan_flags")
    assert lib.silent_abi_version() == 5


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_plan_flags_validation_on_the_host_side():
    """Unknown flag bits -> invalid, float64 with 3 channels -> unsupported, the flags round-trip; float64 plans' host code."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    lib = B.build_host_asan()
    rt_lib = B.asan_runtime()
    if rt_lib is None:
        pytest.skip("the ROCm LLVM has no shared asan runtime")
    env = dict(os.environ, LD_PRELOAD=rt_lib, SILENT_LIB_PATH=lib, ASAN_OPTIONS="detect_leaks=0:alloc_dealloc_mismatch=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gray_f64_host_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "gray float64 host worker ok" in p.stdout, p.stdout[-4000:]
    assert "AddressSanitizer" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]


@pytest.mark.parametrize("kwargs", [dict(accumulation="float16"), dict(accumulation="double"), dict(accumulation=None),
                                    dict(mode="rgb", accumulation="float64")])
def test_pipeline_refuses_bad_accumulation_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match="accumulation"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def _ordered(a):
    """float32 -> int64 keys whose differences count ulps across the sign boundary too."""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def separable_f64(plane, y0, x0, ch, cw, zh, zw):
    """The F64 kernels' pyramid order: float64 weights, vertical taps then horizontal taps, rounded to float32 once."""
    import silent_oracle as so
    _, iy, wy = so.zoom_axis_table(ch, zh)
    _, ix, wx = so.zoom_axis_table(cw, zw)
    p = plane[y0:y0 + ch, x0:x0 + cw].astype(np.float64)
    v = np.zeros((zh, cw))
    for a in range(6):
        v += wy[:, a][:, None] * p[iy[:, a], :]
    out = np.zeros((zh, zw))
    for b in range(6):
        out += wx[:, b][None, :] * v[:, ix[:, b]]
    return out.astype(np.float32)


@pytest.mark.parametrize("scale,n_levels", [(2.0, 5), (float(np.e) ** .5, 6)])
def test_separable_float64_spline_is_within_one_ulp_of_the_oracle(scale, n_levels):
    import c_oracle as co
    from pysilent_amd.util.zoom.from_image import classic_levels
    h, w = 1080, 1920
    total = differ = 0
    for seed in range(2):
        plane = (np.random.default_rng(seed).random((h, w)) * 255.0).astype(np.float32)
        for (y0, x0, ch, cw, zh, zw, oh, ow) in classic_levels((h, w), scale, n_levels):
            want = co.zoom_level(plane[:, :, None], y0, x0, ch, cw, zh, zw, oh, ow)[:, :, 0]
            got = separable_f64(plane, y0, x0, ch, cw, zh, zw)
            zr, zc = min(zh, oh), min(zw, ow)
            d = np.abs(_ordered(got[:zr, :zc]) - _ordered(want[:zr, :zc]))
            assert d.max() <= 1, "level %dx%d: %d ulps" % (zh, zw, d.max())
            total += d.size
            differ += int((d != 0).sum())
    share = differ / total
    print("scale %.4f: %d of %d elements differ by 1 ulp (share %.2e)" % (scale, differ, total, share))
    assert share <= 1e-5
