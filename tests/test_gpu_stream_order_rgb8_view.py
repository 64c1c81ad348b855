"""The stream contract of silent_pyramid_rgb8_view_dev (include/silent_hip.h: the _dev form is stream-ordered and asynchronous), through
the harness of tests/stream_order.py: the call runs on a held stream of the caller's, behind the producer of its frames and in front
of an overwriter, and must return the bits of the quiet call -- with the hold still pending when it returns, on torch's current
stream (asserted by the harness's proxy for every silent_*_dev call), and given the parent buffer itself, not a packed copy.
The cases are those of tests/test_gpu_write_coverage_rgb8_view.py: a region of larger frames and BGRA without its fourth byte."""
import pytest

import stream_order as so
import test_gpu_stream_order as tso
import test_gpu_write_coverage_rgb8_view as tr

pytestmark = pytest.mark.gpu

# silent_pyramid_rgb8_view_dev takes a silent_frame_view in host memory: tests/test_gpu_stream_order.py finds it by its signature
# (test_host_arguments_are_dead_at_return) and asks for a case that reaches it -- named here, when the suite is collected, so that the
# scenario of that file runs on the new entry point as it does on the others
tso.HOST_ARG_CASES[tr.CASES[0].id] = tr.CASES[0]
tso.REACHED_BY["pyramid_rgb8_view"] = tr.CASES[0].id


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
def test_rgb8_view_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert len(bufs.calls) == 2
    for i in range(2):
        with h.watching() as w:
            bufs.calls[i]()
        assert [r["name"] for r in w.records] == ["silent_pyramid_rgb8_view_dev"]
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


def test_rgb8_view_two_streams_with_different_inputs(rt, h):
    case = tr.CASES[0]
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    for i in range(2):
        so.scenario_two_streams(h, subj, i, pair)
    so.scenario_two_streams(h, subj, 1, pair, hold_both=True)
