"""The stream contract of the *_dev entry points (include/silent_hip.h:19-28; the harness: tests/stream_order.py; the cases: those of
tests/write_coverage_cases.py, every call on its own, no new shapes).

Everywhere else in the suite a call runs on the legacy default stream with the device synchronised around it, where a launch on the
wrong stream, a table read after return or a missing drain gives the same bits.  Here every call runs on a stream of the caller's
that is held busy, behind the producer of its inputs and in front of an overwriter, and must return the bits of the quiet call:

  1  producer ahead, second call right behind, overwriter last -- every call of every case;
  2  two streams, different inputs: the workspace changes hands -- the workspace cases and one case per other family, with S held
     and with both streams held (released together, so that calls the library failed to order would meet in the workspace);
  3  the host-pointer form while a device form is pending -- the workspace cases;
  4  host arguments overwritten the moment the call returns -- every silent_*_dev with an argument in host memory;
  5  LineEndPipeline.step on a caller's stream, frames produced and overwritten on it.

Run with -s for the hold D of every sequence and the `verified` flags of the two streams.

Out of scope: the displayer (a stream, graph and pinned slots of its own), HIP-graph capture of library calls, multi-GPU, bench.py.
No timing is asserted: `pending` is a stream query."""
import ctypes as C

import numpy as np
import pytest

import plan_geometry as pg
import stream_order as so
import test_gpu_write_coverage_strided as tvs
import test_gpu_write_coverage_u16 as tvu
import write_coverage as wc
import write_coverage_cases as wcc

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


# ----------------------------------------------------------------------------- the harness has teeth

def test_the_harness_reports_each_violation(rt, h):
    """Scenarios 1 and 4 with torch ops playing the library: a correct op passes; an op on the default stream and one on a side
    stream that never waited for S read the decoy; an asynchronous copy from a pinned host array sees what the harness wrote there
    at return; an op that synchronises is reported by the pending check."""
    import torch
    if not h.verified:
        pytest.skip("pick_concurrent_stream found no stream that runs beside the default stream in 10 tries: a hold on S would "
                    "hold the default stream too")
    x = np.arange(1, 2 * 7 * 13 * 3 + 1, dtype=np.float32).reshape(2, 7, 13, 3)
    side = torch.cuda.Stream(h.dev)
    weights = torch.full(x.shape, 2.0).pin_memory()

    def on(stream):
        def calls(rt, t):
            def run():
                with torch.cuda.stream(stream() if stream else torch.cuda.current_stream(h.dev)):
                    return (t * 2 + 1,)
            return [run]
        return calls

    def synchronising(rt, t):
        def run():
            torch.cuda.synchronize(h.dev)
            return (t * 2 + 1,)
        return [run]

    def from_pinned(rt, t):
        def run():
            w = torch.empty_like(t)
            w.copy_(weights, non_blocking=True)
            return (t * w,)
        return [run]

    def scenario1(calls):
        return so.scenario_producer_call_overwriter(h, so.Subject("torch op", calls, [x]), 0, library=False)

    scenario1(on(None))
    with pytest.raises(AssertionError, match=r"first call behind the producer, against the quiet call on a: buffer result 0: \d+ of 546 elements differ"):
        scenario1(on(lambda: torch.cuda.default_stream(h.dev)))
    with pytest.raises(AssertionError, match=r"first call behind the producer, against the quiet call on a: buffer result 0: \d+ of 546 elements differ"):
        scenario1(on(lambda: side))
    with pytest.raises(AssertionError, match=r"synchronised: call \[0, 1\] of the sequence returned only after the hold had run out"):
        scenario1(synchronising)
    subj = so.Subject("torch op", from_pinned, [x])
    bufs = so.Buffers(rt, subj, subj.a)
    so.scenario_host_arguments(h, subj, 0, bufs)                                    # nobody overwrites the array: passes
    with pytest.raises(AssertionError, match=r"host arguments overwritten at return, against the quiet call with the original arguments: "
                                             r"buffer result 0: 546 of 546 elements differ"):
        so.scenario_host_arguments(h, subj, 0, bufs, host_arrays=[weights.numpy()])
    assert (weights.numpy() == 2.0).all()


def test_the_direct_routes_make_the_catalogues_calls(rt, h):
    """stream_order.DIRECT replaces closures that copy their input (abs(x), f32 * 0) by the same library call on the buffer itself:
    the quiet results are those of the catalogue's closures."""
    cases = {c.id: c for c in wcc.CASES}
    for cid in sorted(so.DIRECT):
        case = cases[cid]
        calls = case.calls(rt, *[wcc.on_device(rt, v) for v in case.inputs()])
        want = []
        for call in calls:
            h.sync()
            want.append(wc.specified(call()))
            h.sync()
        got = so.quiet(h, so.subject(case), "a")
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            wc.assert_same_bits(g, w, "%s call %d: the direct route against the catalogue's closure" % (cid, i))


# ----------------------------------------------------------------------------- scenarios 1 - 3: the catalogue

@pytest.mark.parametrize("case", wcc.CASES, ids=wcc.IDS)
def test_calls_behind_a_producer_and_before_an_overwriter(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert bufs.calls
    for i in range(len(bufs.calls)):
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


FA = "%dx%d" % pg.FA
# one case without a context workspace per family: pointwise, conv, regulate, gray pass, pyramid, RGB chain
OTHER_FAMILIES = ["pad_inwards", "conv2d_same-3x3x3x4", "regulate-7x7x3x3", "gray_pass-ratio2_3-%s-K4" % FA, "plan-nested_316-c3",
                  "rgb_line_end-symmetric"]
WORKSPACE = [c for c in wcc.CASES if c.workspace]
TWO_STREAMS = WORKSPACE + [c for c in wcc.CASES if c.id in OTHER_FAMILIES]
assert len(TWO_STREAMS) == len(WORKSPACE) + len(OTHER_FAMILIES)


@pytest.mark.parametrize("case", TWO_STREAMS, ids=[c.id for c in TWO_STREAMS])
def test_two_streams_with_different_inputs(rt, h, case):
    subj = so.subject(case)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    for i in range(len(pair[0].calls)):
        so.scenario_two_streams(h, subj, i, pair)
        so.scenario_two_streams(h, subj, i, pair, hold_both=True)


@pytest.mark.parametrize("case", WORKSPACE, ids=[c.id for c in WORKSPACE])
def test_host_form_while_a_device_form_is_pending(rt, h, case):
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.a)
    host_calls = subj.calls(rt, *[wcc.on_host(rt, v) for v in subj.b])
    assert len(host_calls) == len(bufs.calls)
    for i in range(len(bufs.calls)):
        so.scenario_host_form_behind_device_form(h, subj, i, bufs, host_calls)


# ----------------------------------------------------------------------------- scenario 4: host arguments are dead at return

def _parts_calls(rt, f32):
    """silent_gray_pass_parts_dev: the two halves of one pass, one call each (the wrappers reach it through LineEndPipeline only)."""
    plan = wcc.plan_of(rt, ("gray", "ratio2_3", pg.FA), pg.FA, 1, wcc.gray_family_levels("ratio2_3", pg.FA))

    def run():
        op = plan._frames(f32)
        n = op.n_frames
        (pyr, pp), (cso, cp), (endo, ep) = [op.empty(n * plan.frame_px * ch) for ch in (1, 1, 4)]
        for parts in (1, 2):
            cs_k, bank = [np.ascontiguousarray(np.asarray(k, np.float64).astype(np.float32)) for k in wcc._gray_weights(4)]
            op.call("gray_pass_parts", plan.handle, op.ptr, n, C.c_void_p(cs_k.ctypes.data), C.c_void_p(bank.ctypes.data), 4, 255.0, pp, cp, ep, parts)
        return pyr, cso, endo
    return [run]


PARTS = wcc.Case("gray_pass_parts-ratio2_3-%s-K4" % FA, _parts_calls, lambda: wcc._plan_inputs(pg.FA, 1, 500)()[:1], 0)
HOST_ARG_CASES = {c.id: c for c in wcc.CASES + tvs.CASES + tvu.CASES + [PARTS]}
# entry point -> a case whose calls reach it
REACHED_BY = {"conv2d_same": "conv2d_same-3x3x3x4", "regulate": "regulate-7x7x3x3", "gray_line_end": "gray_line_end-K4",
              "pad_inwards": "pad_inwards", "value_from_color": "value_from_color", "bw_from_color": "bw_from_color",
              "nms3x3": "nms3x3-product", "top_value_points": "top_value_points", "affine_clip": "affine_clip",
              "select_peaks": "select_peaks-c3", "resize_nearest": "resize_nearest", "centroids": "centroids",
              "boosting_step": "boosting_step", "max_value_indices_region": "max_value_indices_region-few_windows",
              "select_keypoints": "select_keypoints-few_windows", "rgb_line_end": "rgb_line_end-symmetric",
              "rgb_keypoints": "rgb_keypoints-symmetric-sparse", "gray_pass_parts": PARTS.id}
REACHED_BY.update({n: "gray_pass-ratio2_3-%s-K4" % FA for n in ("gray_pass", "gray_pass_h", "gray_pass_u8", "gray_pass_u8x3")})
REACHED_BY.update({n: "gray_keypoints-ratio2_3-%s-K4" % FA for n in ("gray_keypoints", "gray_keypoints_u8", "gray_keypoints_u8x3")})
REACHED_BY.update({n: tvs.CASES[0].id for n in ("pyramid_view", "gray_pass_view", "gray_keypoints_view")})
REACHED_BY.update({n: tvu.CASES[0].id for n in ("gray_pass_u16", "gray_keypoints_u16", "pyramid_view16", "gray_pass_view16", "gray_keypoints_view16")})


@pytest.mark.parametrize("name", so.dev_entry_points_with_host_arguments())
def test_host_arguments_are_dead_at_return(rt, h, name):
    """Every silent_*_dev that takes weights, silent_extent tables, a parameter block or a frame view in host memory (found by its
    signature: a new entry point without a case in REACHED_BY fails here)."""
    short = name[len("silent_"):-len("_dev")]
    assert short in REACHED_BY, "%s takes arguments in host memory: name a case that reaches it in REACHED_BY" % name
    case = HOST_ARG_CASES[REACHED_BY[short]]
    subj = so.subject(case)
    bufs = so.Buffers(rt, subj, subj.a)
    seen = {}
    for i in range(len(bufs.calls)):
        for r in so.scenario_host_arguments(h, subj, i, bufs):
            seen.setdefault(r["name"], []).append(r["clobbered"])
    assert name in seen, "%s: no call of %s reached %s (%s)" % (case.id, case.id, name, sorted(seen))
    assert all(seen[name]), "%s: nothing was overwritten behind a call of %s" % (case.id, name)
    print("stream-order host arguments: %s: %s" % (name, "; ".join(seen[name][0])))


# ----------------------------------------------------------------------------- scenario 5: pipelines

PIPELINES = {"gray-keypoints-selection": dict(mode="gray", keypoints=True, selection=True), "rgb-selection": dict(mode="rgb", selection=True)}
PIPE_BUFFERS = ("pyr", "cs", "end", "orient", "line_end", "value", "peak_value")


def _snapshot(pipe):
    """Copies of every buffer a step writes, made on torch's current stream (outputs() reads the counts back: a synchronisation)."""
    maps = [getattr(pipe, n).clone() for n in PIPE_BUFFERS if getattr(pipe, n, None) is not None]
    return tuple(maps) + (wc.Rows(pipe.kp_idx.clone(), pipe.kp_counts.clone()),)


def _outputs(pipe):
    out = pipe.outputs()
    named = []
    for k in sorted(out):
        v = out[k]
        if k == "keypoints":
            named += [("keypoints of frame %d" % f, wc.to_numpy(a)) for f, a in enumerate(v)]
        else:
            named.append((k, wc.to_numpy(v)))
    return named


@pytest.mark.parametrize("name", sorted(PIPELINES))
def test_pipeline_steps_on_a_callers_stream(rt, h, name):
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    hw, c = pg.FA, 1 if PIPELINES[name]["mode"] == "gray" else 3
    pipe = LineEndPipeline(hw, batch=2, device=0, placement=None, overlap=False, **PIPELINES[name])
    # (the second batch at half the amplitude: other extrema, another threshold -- see stream_order.shuffled)
    a, b = [torch.from_numpy(np.stack([wcc.noise(hw + (c,), 40 + 10 * s + f) for f in range(2)]) * np.float32(1.0 - 0.5 * s)).to(h.dev)
            for s in range(2)]
    frames = torch.empty_like(a)
    dec = (a + b) * 0.25
    want, want_out = [], []
    for x in (a, b):
        frames.copy_(x)
        h.sync()
        pipe.step(frames)
        h.sync()
        want.append(wc.specified(_snapshot(pipe)))
        want_out.append(_outputs(pipe))
    h.sync()

    def seq(d):
        with torch.cuda.stream(h.S):
            if d:
                h.hold(d)
            frames.copy_(a, non_blocking=True)
            pipe.step(frames)
            pa, sa = h.pending(), _snapshot(pipe)
            frames.copy_(b, non_blocking=True)
            pipe.step(frames)
            pb, sb = h.pending(), _snapshot(pipe)
            frames.zero_()
        return (sa, sb), [pa, pb]

    what = "pipeline %s" % name
    (sa, sb), _, _ = h.run_held(what, seq, lambda: frames.copy_(dec), asserted=(0, 1))
    wc.assert_same_bits(wc.specified(sa), want[0], what + ": first step behind the producer of its frames, against the quiet step")
    wc.assert_same_bits(wc.specified(sb), want[1], what + ": second step, on overwritten frames, against the quiet step")
    with torch.cuda.stream(h.S):
        wc.assert_same_bits(_outputs(pipe), want_out[1], what + ": outputs() after the second step, against the quiet pipeline's")
