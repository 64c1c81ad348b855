"""The stream contract of silent_pyramid_yuv16_dev and silent_yuv16_to_rgb_dev (include/silent_hip.h: the _dev forms are stream-ordered
and asynchronous), through the harness of tests/stream_order.py: each call runs on a held stream of the caller's, behind the producer
of its surfaces and in front of an overwriter, and must return the bits of the quiet call -- with the hold still pending when it
returns, on torch's current stream (asserted by the harness's proxy for every silent_*_dev call), and given the surfaces themselves,
not a copy.  The cases are those of tests/test_gpu_write_coverage_yuv16.py (I010 and Y210)."""
import ctypes as C

import pytest

import stream_order as so
import test_gpu_write_coverage_yuv16 as ty

pytestmark = pytest.mark.gpu

# The harness asks whether a call was handed the input buffer itself by looking at its pointer arguments (stream_order._pointers); the
# three plane pointers of a 16-bit YUV call travel inside a silent_yuv16_frames, a struct that module does not know.  They are added here,
# when the suite is collected -- every other argument type is answered by the function as it stands.
_pointers_before = so._pointers


def _pointers_with_yuv16(argtypes, args):
    from pysilent_amd import _lib
    out = _pointers_before(argtypes, args)
    for t, v in zip(argtypes[1:-1], args[1:-1]):
        if t is _lib._y16p and v is not None:
            out += [int(v.contents.y or 0), int(v.contents.u or 0), int(v.contents.v or 0)]
    return out


so._pointers = _pointers_with_yuv16
NAMES = ["silent_pyramid_yuv16_dev", "silent_yuv16_to_rgb_dev"]


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


@pytest.fixture(scope="module")
def h(rt):
    return so.Harness(rt)


@pytest.mark.parametrize("case", ty.CASES, ids=ty.IDS)
def test_yuv16_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert len(bufs.calls) == 2
    for i in range(2):
        with h.watching() as w:
            bufs.calls[i]()
        assert [r["name"] for r in w.records] == [NAMES[i]]
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


@pytest.mark.parametrize("which", (0, len(ty.CASES) // 2), ids=["i010", "y210"])
def test_yuv16_two_streams_with_different_inputs(rt, h, which):
    case = ty.CASES[which]
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    for i in range(2):
        so.scenario_two_streams(h, subj, i, pair)
    so.scenario_two_streams(h, subj, 1, pair, hold_both=True)


def test_the_struct_is_dead_at_return(rt, h):
    """The silent_yuv16_frames of a _dev call lies in host memory: zeroed right after the call returns, while the stream is still held,
    the call still gives the quiet call's bits (the kernels got the struct by value)."""
    import numpy as np
    import torch
    from pysilent_amd import _lib
    case = ty.CASES[len(ty.CASES) // 2]
    layout, _, hw = ty._parse(case)
    assert layout == "y210"
    surfaces = torch.from_numpy(np.array(case.inputs()[0])).cuda(0)
    planes = ty._planes(layout, hw, surfaces)
    m, oy, oc = rt.p010_coefficients(depth=10)
    want = rt.yuv16_to_rgb(planes, hw, "yuv422p10msb")
    torch.cuda.synchronize()
    args = rt.yuv16_frames_of(planes, hw, "yuv422p10msb", m, oy, oc)[0]
    out = torch.zeros_like(want)
    ctx = rt.get_context(0)
    struct = _lib.yuv16_ptr(args)
    h.sync()
    h.hold(20000)
    ctx.check(_lib.load().silent_yuv16_to_rgb_dev(ctx.handle, struct, 2, hw[0], hw[1], C.c_void_p(out.data_ptr()), C.c_void_p(h.S.cuda_stream)))
    pending = h.pending()
    C.memset(C.addressof(struct.contents), 0, C.sizeof(struct.contents))
    h.sync()
    assert pending, "the call returned only after the hold had run out"
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
