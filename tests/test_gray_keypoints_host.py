"""silent_gray_keypoints without a GPU: the ABI, argument validation (the library's host side built without a GPU behind it, as
tests/test_sanitizers.py builds it), and the CPU reference composition the GPU tests compare against (tests/gray_kp_oracle.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, noise_frame, structured_frame


def test_gray_keypoints_symbols_are_declared_and_bound():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    for name in ("silent_gray_keypoints", "silent_gray_keypoints_dev"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 5
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    assert "#define SILENT_ABI_VERSION 5" in src


def test_library_exports_gray_keypoints():
    import ctypes
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "silent_gray_keypoints") and hasattr(lib, "silent_gray_keypoints_dev")
    assert lib.silent_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("K", [3, 4, 8])
@pytest.mark.parametrize("selection", [True, False])
def test_oracle_composition_rows_sorted_unique_and_hold_each_levels_maximum(K, selection, kernels):
    import silent_oracle as so
    from gray_kp_oracle import gray_tail
    frame = structured_frame(K, 64, 96, 1) if selection else noise_frame(K, 64, 96, 1)
    pyr = so.classic_pyramid(frame, 2.0, 3)
    ends = [end[0] for _, end in so.gray_line_end_pass(pyr, kernels["cs_gray"], kernels["end%d" % K])]
    rows, values, peaks = gray_tail(ends, pad=2, selection=selection, top_percent=0.1)
    assert rows.ndim == 2 and rows.shape[1] == 4 and len(rows) > 0
    keys = [tuple(r) for r in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert (rows[:, 3] == 0).all()
    for l, v in enumerate(peaks if selection else values):
        y, x = np.unravel_index(int(np.argmax(v)), v.shape)
        assert (l, y, x, 0) in set(keys), "level %d: its global maximum is not a keypoint" % l


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_argument_validation_on_the_host_side():
    """Bad n_orient, pad < 0, NULL idx with a nonzero cap, a region count that does not match the levels: mapped Python errors."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    lib = B.build_host_asan()
    rt_lib = B.asan_runtime()
    if rt_lib is None:
        pytest.skip("the ROCm LLVM has no shared asan runtime")
    env = dict(os.environ, LD_PRELOAD=rt_lib, SILENT_LIB_PATH=lib, ASAN_OPTIONS="detect_leaks=0:alloc_dealloc_mismatch=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gray_kp_host_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "gray keypoints host worker ok" in p.stdout, p.stdout[-4000:]
    assert "AddressSanitizer" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]
