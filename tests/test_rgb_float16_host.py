"""float16 storage of the RGB chain's maps, everything that needs no GPU: the rgb_storage keyword and its refusals, the constraints it
was shaped by (storage="float16" keeps raising on mode "rgb", LineEndPipeline.__init__ keeps its parameter list), the four new symbols
in the header, the bindings and the library, and every refusal of the four entry points in order -- a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/rgb_h_host_main.cpp), run as a child process."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["silent_rgb_line_end_h", "silent_rgb_line_end_h_dev", "silent_rgb_keypoints_h", "silent_rgb_keypoints_h_dev"]


def _no_torch(monkeypatch):
    import torch

    def no_torch(*a, **k):
        raise AssertionError("torch work before the refusal")
    monkeypatch.setattr(torch, "device", no_torch)


@pytest.mark.parametrize("kw, message", [
    (dict(mode="rgb", rgb_storage="float8"), "rgb_storage must be 'float32' or 'float16', got 'float8'"),
    (dict(mode="rgb", rgb_storage=None), "rgb_storage must be 'float32' or 'float16', got None"),
    (dict(mode="gray", rgb_storage="float16"), "rgb_storage='float16' is for mode 'rgb' (the gray pass takes storage='float16')"),
    (dict(mode="rgb", rgb_storage="float16", selection=True, keep_selection_maps=True),
     "rgb_storage='float16' does not combine with keep_selection_maps=True (the top / peaks maps come from the float32 per-op kernels)")])
def test_the_keyword_is_refused_before_any_gpu_work(kw, message, monkeypatch):
    from pysilent_amd.pipeline import LineEndPipeline
    _no_torch(monkeypatch)
    with pytest.raises(ValueError) as e:
        LineEndPipeline((64, 96), **kw)
    assert str(e.value) == message


def test_check_rgb_storage():
    from pysilent_amd import _runtime as rt
    assert rt.check_rgb_storage("float32") == "float32" and rt.check_rgb_storage("float16") == "float16"
    assert rt.check_rgb_storage("float32", "gray", True) == "float32"          # the default combines with everything
    with pytest.raises(ValueError, match="rgb_storage must be"):
        rt.check_rgb_storage("half")
    with pytest.raises(ValueError, match="storage must be 'float32' or 'float16', got 'half'"):
        rt.rgb_line_end(None, {}, storage="half")


def test_storage_float16_still_raises_on_mode_rgb(monkeypatch):
    from pysilent_amd.pipeline import LineEndPipeline
    _no_torch(monkeypatch)
    with pytest.raises(ValueError) as e:
        LineEndPipeline((64, 96), mode="rgb", storage="float16")
    assert str(e.value) == "storage='float16' is for mode 'gray' (the RGB maps are stored as float32)"


def test_the_keyword_belongs_to_the_call_and_init_keeps_its_parameters():
    from pysilent_amd import pipeline
    names = list(inspect.signature(pipeline.LineEndPipeline.__init__).parameters)
    assert pipeline.RGB_STORAGE_KEYWORDS == {"rgb_storage": "float32"}
    assert "rgb_storage" not in names
    assert names[-4:] == ["rgb_frame_format", "nv12_matrix", "nv12_range", "nv12_order"] and names[1:3] == ["frame_hw", "mode"]
    assert len(names) == 36, names
    with pytest.raises(TypeError, match="rgb_storge"):
        pipeline.LineEndPipeline((64, 96), mode="rgb", rgb_storge="float16")


def _declaration(header, name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, "%s is not declared in include/silent_hip.h" % name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_the_new_symbols_are_declared_bound_and_exported():
    """Each with its float32 twin's signature apart from the two map pointers."""
    from pysilent_amd import _lib
    header = open(os.path.join(ROOT, "include", "silent_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        twin = name.replace("_h", "", 1) if name.endswith("_h") else name.replace("_h_dev", "_dev")
        a, b = _declaration(header, name), _declaration(header, twin)
        assert len(a) == len(b)
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert diff == [("uint16_t* orient_out", "float* orient_out"), ("uint16_t* line_end_out", "float* line_end_out")], (name, diff)
        sa, sb = _lib._SIGNATURES[name], _lib._SIGNATURES[twin]
        assert len(sa) == len(sb)
        assert [i for i, (x, y) in enumerate(zip(sa, sb)) if x is not y] == [i for i, x in enumerate(a) if x.startswith("uint16_t*")]
        assert all(sa[i] is _lib._hp for i, x in enumerate(a) if x.startswith("uint16_t*"))
        fn = getattr(lib, name)                                  # exported (hidden visibility otherwise: AttributeError)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(sa)
    assert "#define SILENT_ABI_VERSION" in header


def test_every_refusal_in_order_under_the_sanitizers():
    """tests/rgb_h_host_main.cpp: one translation unit with the library's host side, -fsanitize=address,undefined, its own main."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    env = dict(os.environ, ASAN_OPTIONS="alloc_dealloc_mismatch=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([B.build_host_driver("rgb_h")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "Sanitizer" not in p.stdout and "runtime error" not in p.stdout and "CHECK FAILED" not in p.stdout, p.stdout[-4000:]
    rows = [[c.strip() for c in line.split("|")] for line in p.stdout.strip().split("\n")]
    by = {}
    for r in rows:
        by.setdefault(r[0], []).append(r)
    assert sorted(by) == sorted(NEW)
    for name, rs in by.items():
        who = name[:-4] if name.endswith("_dev") else name
        cases = [r[1] for r in rs]
        assert cases[:2] == ["null_pyr", "null_params"] and cases[-1] == "accepted" and rs[-1][2] == "0"
        assert "blur_not_channel_uniform" in cases and cases.index("blur_not_channel_uniform") > cases.index("negative_pad")
        assert cases.index("bad_flat_policy") > cases.index("blur_not_channel_uniform")
        for r in rs[:-1]:
            assert int(r[2]) < 0 and r[3].startswith(who + ": "), r          # under the new name
        own = {r[1]: r for r in rs}
        assert own["blur_not_channel_uniform"][2] == "-4" and "channel-uniform blur" in own["blur_not_channel_uniform"][3]
        if name.endswith("_dev"):
            assert own["level_too_large"][2] == "-4" and "too large for the pair kernel" in own["level_too_large"][3]
            assert own["odd_orient_address"][2] == "-1" and "2-byte aligned" in own["odd_orient_address"][3]
        if "keypoints" in name:
            assert own["null_line_end"][2] == "-1"                                # required in both forms
