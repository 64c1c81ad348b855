"""The stream contract of silent_pyramid_p010_dev and silent_p010_to_rgb_dev (include/silent_hip.h: the _dev forms are stream-ordered
and asynchronous), through the harness of tests/stream_order.py: each call runs on a held stream of the caller's, behind the producer
of its surfaces and in front of an overwriter, and must return the bits of the quiet call -- with the hold still pending when it
returns, on torch's current stream (asserted by the harness's proxy for every silent_*_dev call), and given the surfaces themselves,
not a copy.  The cases are those of tests/test_gpu_write_coverage_p010.py."""
import ctypes as C

import pytest

import stream_order as so
import test_gpu_write_coverage_p010 as tp

pytestmark = pytest.mark.gpu

# The harness asks whether a call was handed the input buffer itself by looking at its pointer arguments (stream_order._pointers); the
# two plane pointers of a P010 call travel inside a silent_p010_frames, a struct that module does not know.  They are added here, when
# the suite is collected, on top of whatever the function answers by then (tests/test_gpu_stream_order_nv12.py does the same).
_pointers_before = so._pointers


def _pointers_with_p010(argtypes, args):
    from pysilent_amd import _lib
    out = _pointers_before(argtypes, args)
    for t, v in zip(argtypes[1:-1], args[1:-1]):
        if t is _lib._pp and v is not None:
            out += [int(v.contents.y or 0), int(v.contents.uv or 0)]
    return out


so._pointers = _pointers_with_p010
NAMES = ["silent_pyramid_p010_dev", "silent_p010_to_rgb_dev"]


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


@pytest.fixture(scope="module")
def h(rt):
    return so.Harness(rt)


@pytest.mark.parametrize("case", tp.CASES, ids=tp.IDS)
def test_p010_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert len(bufs.calls) == 2
    for i in range(2):
        with h.watching() as w:
            bufs.calls[i]()
        assert [r["name"] for r in w.records] == [NAMES[i]]
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


def test_p010_two_streams_with_different_inputs(rt, h):
    case = tp.CASES[0]
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    for i in range(2):
        so.scenario_two_streams(h, subj, i, pair)
    so.scenario_two_streams(h, subj, 1, pair, hold_both=True)


def test_the_struct_is_dead_at_return(rt, h):
    """The silent_p010_frames of a _dev call lies in host memory: zeroed right after the call returns, while the stream is still held,
    the call still gives the quiet call's bits (the kernels got the struct by value)."""
    import numpy as np
    import torch
    from pysilent_amd import _lib
    case = tp.CASES[0]
    hw = tuple(int(v) for v in case.id.split("-")[2].split("x"))
    surfaces = torch.from_numpy(np.array(case.inputs()[0])).cuda(0)
    planes = tp._planes(hw, surfaces)
    m, oy, oc = rt.p010_coefficients(depth=10)
    want = rt.p010_to_rgb(planes, hw)
    torch.cuda.synchronize()
    args = rt.p010_frames_of(planes, hw, m, oy, oc, 10)[0]
    out = torch.zeros_like(want)
    ctx = rt.get_context(0)
    struct = _lib.p010_ptr(args)
    h.sync()
    h.hold(20000)
    ctx.check(_lib.load().silent_p010_to_rgb_dev(ctx.handle, struct, 2, hw[0], hw[1], C.c_void_p(out.data_ptr()), C.c_void_p(h.S.cuda_stream)))
    pending = h.pending()
    C.memset(C.addressof(struct.contents), 0, C.sizeof(struct.contents))
    h.sync()
    assert pending, "the call returned only after the hold had run out"
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
