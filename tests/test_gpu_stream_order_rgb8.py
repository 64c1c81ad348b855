"""The stream contract of silent_pyramid_rgb8_dev (include/silent_hip.h: the _dev form is stream-ordered and asynchronous), through the
harness of tests/stream_order.py: the call runs on a held stream of the caller's, behind the producer of its frames and in front of
an overwriter, and must return the bits of the quiet call -- with the hold still pending when it returns, on torch's current
stream (asserted by the harness's proxy for every silent_*_dev call), and given the frame buffer itself, not a converted copy.
The cases are those of tests/test_gpu_write_coverage_rgb8.py."""
import pytest

import stream_order as so
import test_gpu_write_coverage_rgb8 as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


@pytest.fixture(scope="module")
def h(rt):
    return so.Harness(rt)


@pytest.mark.parametrize("case", tr.CASES, ids=tr.IDS)
def test_rgb8_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert len(bufs.calls) == 1
    with h.watching() as w:
        bufs.calls[0]()
    assert [r["name"] for r in w.records] == ["silent_pyramid_rgb8_dev"]
    so.scenario_producer_call_overwriter(h, subj, 0, bufs)


def test_rgb8_two_streams_with_different_inputs(rt, h):
    case = tr.CASES[0]
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    so.scenario_two_streams(h, subj, 0, pair)
    so.scenario_two_streams(h, subj, 0, pair, hold_both=True)
