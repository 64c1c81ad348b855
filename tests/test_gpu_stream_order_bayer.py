"""The stream contract of silent_pyramid_bayer_dev and silent_bayer_to_rgb_dev (include/silent_hip.h: the _dev forms are stream-ordered
and asynchronous), through the harness of tests/stream_order.py: each call runs on a held stream of the caller's, behind the producer
of its mosaics and in front of an overwriter, and must return the bits of the quiet call -- with the hold still pending when it
returns, on torch's current stream (asserted by the harness's proxy for every silent_*_dev call), and given the buffers themselves,
not a copy.  The cases are those of tests/test_gpu_write_coverage_bayer.py (a window of sensor images, every second byte)."""
import ctypes as C

import pytest

import stream_order as so
import test_gpu_write_coverage_bayer as tb

pytestmark = pytest.mark.gpu

# The harness asks whether a call was handed the input buffer itself by looking at its pointer arguments (stream_order._pointers); the
# data pointer of a Bayer call travels inside a silent_bayer_frames, a struct that module does not know.  It is added here, when the
# suite is collected -- every other argument type is answered by the function as it stands.
_pointers_before = so._pointers


def _pointers_with_bayer(argtypes, args):
    from pysilent_amd import _lib
    out = _pointers_before(argtypes, args)
    for t, v in zip(argtypes[1:-1], args[1:-1]):
        if t is _lib._byp and v is not None:
            out += [int(v.contents.data or 0)]
    return out


so._pointers = _pointers_with_bayer
NAMES = ["silent_pyramid_bayer_dev", "silent_bayer_to_rgb_dev"]


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


@pytest.fixture(scope="module")
def h(rt):
    return so.Harness(rt)


@pytest.mark.parametrize("case", tb.CASES, ids=tb.IDS)
def test_bayer_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert len(bufs.calls) == 2
    for i in range(2):
        with h.watching() as w:
            bufs.calls[i]()
        assert [r["name"] for r in w.records] == [NAMES[i]]
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


@pytest.mark.parametrize("which", (0, len(tb.CASES) // 2), ids=["window", "second"])
def test_bayer_two_streams_with_different_inputs(rt, h, which):
    case = tb.CASES[which]
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    for i in range(2):
        so.scenario_two_streams(h, subj, i, pair)
    so.scenario_two_streams(h, subj, 1, pair, hold_both=True)


def test_the_struct_is_dead_at_return(rt, h):
    """The silent_bayer_frames of a _dev call lies in host memory: overwritten right after the call returns, while the stream is still
    held, the call still gives the quiet call's bits (the kernels got their argument by value) -- both entry points."""
    import numpy as np
    import torch
    from pysilent_amd import _lib
    case = tb.CASES[len(tb.CASES) // 2]
    layout, family, hw = tb._parse(case)
    assert layout == "second"
    buffers = torch.from_numpy(np.array(case.inputs()[0])).cuda(0)
    m = tb._mosaic(layout, hw, buffers)
    fmt = tb.LAYOUTS[layout]
    import write_coverage_cases as wcc
    plan = wcc.plan_of(rt, ("bayer", family, hw), hw, 3, wcc.gray_family_levels(family, hw))
    want_rgb, want_pyr = rt.bayer_to_rgb(m, hw, fmt), plan.run(m, rgb_frame_format=fmt).data
    torch.cuda.synchronize()
    args = rt.bayer_frames_of(m, hw, fmt)[0]
    ctx, lib = rt.get_context(0), _lib.load()
    for which, want in enumerate((want_rgb, want_pyr)):
        out = torch.zeros_like(want)
        struct = _lib.bayer_ptr(args)
        h.sync()
        h.hold(20000)
        if which == 0:
            ctx.check(lib.silent_bayer_to_rgb_dev(ctx.handle, struct, 2, hw[0], hw[1], C.c_void_p(out.data_ptr()), C.c_void_p(h.S.cuda_stream)))
        else:
            ctx.check(lib.silent_pyramid_bayer_dev(ctx.handle, plan.handle, struct, 2, C.c_void_p(out.data_ptr()), C.c_void_p(h.S.cuda_stream)))
        pending = h.pending()
        C.memset(C.addressof(struct.contents), 0xA5, C.sizeof(struct.contents))
        h.sync()
        assert pending, "the call returned only after the hold had run out"
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
