"""float16 storage of the gray pass's CS and end maps without a GPU: the refusals (before any torch or GPU work), the ABI, the
argument validation of silent_gray_pass_h (the library's host side built without a GPU behind it, under ASan + UBSan), and the
premise of the GPU test's oracle bound: casting the oracle's maps to float16 overflows nowhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, noise_frame, structured_frame


@pytest.mark.parametrize("kwargs", [dict(storage="bfloat16"), dict(storage="half"), dict(storage=None), dict(storage=16),
                                    dict(storage="float16", mode="rgb"), dict(storage="float16", accumulation="float64"),
                                    dict(storage="float16", keypoints=True),
                                    dict(storage="bfloat16", mode="rgb"), dict(storage="bfloat16", accumulation="float64")])
def test_pipeline_refuses_bad_storage_before_any_gpu_work(kwargs):
    from pysilent_amd.pipeline import LineEndPipeline
    with pytest.raises(ValueError, match="storage"):
        LineEndPipeline((64, 96), batch=1, **kwargs)


def test_check_storage():
    from pysilent_amd import _runtime
    assert _runtime.check_storage("float32") == "float32" and _runtime.check_storage("float16") == "float16"
    assert _runtime.check_storage("float32", "rgb", "float64", True) == "float32"     # (storage off: nothing of it is refused)
    for args in (("bfloat16",), ("uint8",), (None,), ("float16", "rgb"), ("float16", "gray", "float64"),
                 ("float16", "gray", "float32", True)):
        with pytest.raises(ValueError, match="storage"):
            _runtime.check_storage(*args)
    # the name is checked first: an unknown name is reported as such whatever else is wrong
    with pytest.raises(ValueError, match="must be 'float32' or 'float16'"):
        _runtime.check_storage("bfloat16", "rgb", "float64", True)


def test_packed_pyramid_carries_a_dtype():
    from pysilent_amd._runtime import PackedPyramid
    ext = [(4, 6), (2, 3)]
    p = PackedPyramid(np.arange(2 * 30 * 3, dtype=np.float16), ext, 3, 2, dtype=np.float16)
    assert p.dtype == np.float16 and p.data.dtype == np.float16 and p.level(1).shape == (2, 2, 3, 3) and p.level(1).dtype == np.float16
    assert p.like(1).data.dtype == np.float16 and p.like(1).dtype == np.float16
    q = PackedPyramid(np.zeros(2 * 30, np.float64), ext, 1, 2)
    assert q.dtype == np.float32 and q.data.dtype == np.float32 and q.like(2).data.dtype == np.float32
    with pytest.raises(ValueError, match="dtype"):
        PackedPyramid(np.zeros(60), ext, 1, 2, dtype=np.uint8)


def test_float16_symbols_are_declared_bound_and_exported():
    from pysilent_amd import _lib
    import test_abi
    declared = test_abi.declared_symbols()
    half = ctypes.POINTER(ctypes.c_uint16)
    for name, n_args in (("silent_gray_pass_h", 11), ("silent_gray_pass_h_dev", 13)):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
        sig = _lib._SIGNATURES[name]
        assert len(sig) == n_args and sig[9] is half and sig[10] is half     # cs_out, end_out
        assert sig[8] is ctypes.c_void_p                                       # pyr stays a float32 map
    assert _lib._SIGNATURES["silent_gray_pass_h_dev"][11] is ctypes.c_uint       # parts
    assert _lib.ABI_VERSION == 5
    src = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    assert "#define SILENT_ABI_VERSION 5" in src
    for name in ("silent_gray_pass_h", "silent_gray_pass_h_dev"):
        assert "uint16_t* cs_out, uint16_t* end_out" in src[src.index("int " + name + "("):][:400]
    p = _lib.half_ptr(0x1000)
    assert isinstance(p, half) and ctypes.cast(p, ctypes.c_void_p).value == 0x1000 and _lib.half_ptr(None) is None


def test_library_exports_the_float16_symbols():
    from pysilent_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "pysilent_amd", "csrc", "build.py")])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "silent_gray_pass_h") and hasattr(lib, "silent_gray_pass_h_dev")
    assert lib.silent_abi_version() == 5


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_gray_pass_h_validation_on_the_host_side():
    """NULL plan / pointers -> invalid; float64 plan, 3-channel plan, bad n_orient -> unsupported; NULL cs_out or end_out work;
    the host-pointer form's staging: no ASan / UBSan report."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    lib = B.build_host_asan()
    rt_lib = B.asan_runtime()
    if rt_lib is None:
        pytest.skip("the ROCm LLVM has no shared asan runtime")
    env = dict(os.environ, LD_PRELOAD=rt_lib, SILENT_LIB_PATH=lib, ASAN_OPTIONS="detect_leaks=0:alloc_dealloc_mismatch=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gray_f16_host_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "gray float16 host worker ok" in p.stdout, p.stdout[-4000:]
    assert "AddressSanitizer" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]


def _oracle_maps(frame, levels, K):
    import c_oracle as co
    from pysilent_amd.pipeline import default_constants
    consts = default_constants("gray", K)
    cs_k, end_k = np.ascontiguousarray(consts["cs"], np.float32), np.ascontiguousarray(consts["end"], np.float32)
    for l in levels:
        lev = co.zoom_level(frame, *l)[:, :, 0]
        cs, end = co.gray_line_end_level(lev[None, :, :, None], cs_k, end_k, 255.0)
        yield cs[0, :, :, 0], end[0]


@pytest.mark.parametrize("case", ["config1", "noise_1080p", "structured_1080p"])
def test_casting_the_oracle_maps_to_float16_overflows_nowhere(case):
    """The bound of the GPU test (B32 + half a float16 ulp) assumes a finite float16 value wherever the oracle's is finite."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    if case == "config1":
        hw, levels, frame, K = (480, 640), classic_levels((480, 640), 2.0, 3), noise_frame(1, 480, 640, 1), 4
    else:
        hw, levels, K = (1080, 1920), classic_levels((1080, 1920), 2.0, 5), 4
        frame = (noise_frame if case == "noise_1080p" else structured_frame)(2, 1080, 1920, 1)
    top = 0.0
    for cs, end in _oracle_maps(frame, levels, K):
        for m in (cs, end):
            with np.errstate(over="ignore"):
                h = m.astype(np.float16)
            assert np.array_equal(np.isinf(h), np.isinf(m)), "%s: float16 overflow where the float32 map is finite" % case
            assert np.array_equal(np.isnan(h), np.isnan(m))
            top = max(top, float(np.nanmax(m)))
    print("%s: largest oracle value %.6g (float16 max 65504)" % (case, top))
    assert top < 65504.0
