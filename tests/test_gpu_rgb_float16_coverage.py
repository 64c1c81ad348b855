"""Write coverage and stream contract of the float16-storage RGB entry points (silent_rgb_line_end_h[_dev], silent_rgb_keypoints_h[_dev]):
the harnesses of tests/write_coverage.py and tests/stream_order.py on the geometry of tests/test_gpu_rgb_float16.py.  The guards lie
directly around every result, the float16 maps at the weakest placement (orient 2-byte, line_end 16-byte aligned): no byte outside
[ptr, ptr + 6 * px * frames) may change -- including the byte pair next to a row end that lies on a 2-byte boundary only."""
import ctypes as C

import numpy as np
import pytest

import stream_order as so
import test_gpu_rgb_float16 as t16
import test_gpu_stream_order as tso
import test_gpu_write_coverage as tg
import write_coverage as wc
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _half_maps(rt, op, want):
    from pysilent_amd import _lib
    outs, ptrs = {}, {}
    for name in ("orient", "line_end"):
        if name in want:
            outs[name], p = op.empty(op.n_frames * op.frame_px * 3, np.float16)
            ptrs[name] = _lib.half_ptr(p.value)
        else:
            outs[name], ptrs[name] = None, None
    return outs, ptrs


def _wrap_half(rt, op, a):
    return rt.PackedPyramid(a, op.extents, 3, op.n_frames, dtype=np.float16)


def _line_end_h_calls(rt, x):
    """Every output set of silent_rgb_line_end_h[_dev], on the reference's weights (symmetric form) and the dense form."""
    def call(name, want):
        def run():
            res = rt.rgb_line_end(x, t16._weights(name), want=want, storage="float16")
            return tuple(res[n] for n in want)
        return run
    wants = (("orient", "line_end", "value"), ("line_end", "value"), ("orient",), ("value",))
    return [call("reference", w) for w in wants] + [call("dense", wants[0])]


def _keypoints_h_calls(rt, x):
    """silent_rgb_keypoints_h[_dev] with and without the optional outputs (without a value map it lives in the context workspace)."""
    def call(name, optional):
        def run():
            op = rt._Operand(x, channels=3)
            prm, keep = wcc._chain_params(name) if name != "reference" else _reference_params()
            cap = op.frame_px
            maps, hp = _half_maps(rt, op, ("orient", "line_end") if optional else ("line_end",))
            (value, vptr), (pv, pptr) = (op.alloc(1), op.alloc(1)) if optional else ((None, None), (None, None))
            idx, iptr = op.empty((op.n_frames, cap, 4), np.int64)
            counts, cptr = op.empty(op.n_frames, np.int64)
            op.call("rgb_keypoints_h", op.ptr, *op.geom(), C.byref(prm), 0.1, wcc._regions(op, None), hp["orient"], hp["line_end"], vptr, pptr,
                    iptr, cap, cptr)
            res = [_wrap_half(rt, op, maps[n]) for n in ("orient", "line_end") if maps[n] is not None]
            res += [op.wrap(m, 1) for m in (value, pv) if m is not None]
            return tuple(res) + (wc.Rows(idx, counts),)
        return run
    return [call("reference", True), call("reference", False), call("dense", True)]


def _reference_params():
    from pysilent_amd import _lib
    ks = {n: np.ascontiguousarray(np.asarray(t16._weights("reference")[n], np.float64).astype(np.float32)) for n in ("rgc", "rgby", "stripe", "blur", "end")}
    fp = C.POINTER(C.c_float)
    return _lib.RgbChainParams(*[ks[n].ctypes.data_as(fp) for n in ("rgc", "rgby", "stripe", "blur", "end")], 1.0, 0.1, _lib.FLAT_IEEE, 255.0, 2), ks


def _inputs():
    rng = np.random.default_rng(160)
    return [wcc.Packed([(rng.random((t16.N_FRAMES, h, w, 3)) * 255.0).astype(np.float32) for h, w in t16.EXTENTS])]


_PX = t16.N_FRAMES * t16.FRAME_PX
LINE_END_H = wcc.Case("rgb_line_end_h", wcc.each(_line_end_h_calls), _inputs, _PX * 16 + 4096)
KEYPOINTS_H = wcc.Case("rgb_keypoints_h", wcc.each(_keypoints_h_calls), _inputs, _PX * 52 + 4096, workspace=True)
CASES = [LINE_END_H, KEYPOINTS_H]
# tests/test_gpu_stream_order.py finds every silent_*_dev with a host-memory argument by its signature and asks for a case that reaches
# it: both new _dev entry points take silent_extent tables and the parameter block.  Named here, when the suite is collected.
for _c, _short in ((LINE_END_H, "rgb_line_end_h"), (KEYPOINTS_H, "rgb_keypoints_h")):
    tso.HOST_ARG_CASES[_c.id] = _c
    tso.REACHED_BY[_short] = _c.id


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_host_form_does_not_return_stale_arena_bytes(rt, case):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, case)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_results_do_not_depend_on_the_previous_call(rt, case):
    tg.test_results_do_not_depend_on_the_previous_call(rt, case)


@pytest.fixture(scope="module")
def h(rt):
    return so.Harness(rt)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    with h.watching() as w:
        bufs.calls[0]()
    assert [r["name"] for r in w.records] == ["silent_%s_dev" % case.id]
    for i in range(len(bufs.calls)):
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_two_streams_and_the_host_form_behind_a_device_form(rt, h, case):
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    so.scenario_two_streams(h, subj, 0, pair)
    so.scenario_two_streams(h, subj, 0, pair, hold_both=True)
    host_calls = subj.calls(rt, *[wcc.on_host(rt, v) for v in subj.b])
    so.scenario_host_form_behind_device_form(h, subj, 0, pair[0], host_calls)
