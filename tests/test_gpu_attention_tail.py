"""silent_attention_tail[_dev], _runtime.attention_tail and LineEndPipeline(attention=True) on the GPU.

The definition is the per-op sequence of include/silent_hip.h (affine_clip, centroids, resize_nearest, boosting_step: LineEndDisplayer._launch
applied to a packed pyramid), so the first comparison is BIT FOR BIT -- as uint32, NaNs count -- on every geometry x region of
tests/test_attention_tail_host.py, both channel counts, the three recovery modes, five successive calls with the state carried on both
sides.  Then: the CPU oracle on geometry A, frame slots as streams, the pipeline against its own attention=False twin and against the
per-op displayer, the tuners, write coverage and the stream contract (the harnesses of tests/write_coverage.py and tests/stream_order.py)."""
import numpy as np
import pytest

import silent_oracle as oracle
import stream_order as so
import test_attention_tail_host as th
import test_gpu_stream_order as tso
import test_gpu_write_coverage as tg
import write_coverage as wc
import write_coverage_cases as wcc
from conftest import assert_close, noise_frame, structured_frame

pytestmark = pytest.mark.gpu
RTOL = 1e-5
CONSTANT, INPUT = 1, 2
RESULTS = ("centroids", "centroids2", "fired", "update")


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def u32(a):
    a = getattr(a, "data", a) if type(a).__name__ == "PackedPyramid" else a
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same_bits(got, want, what):
    got, want = u32(got), u32(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not bad.size, "%s: %d of %d elements differ, first at %d (%#x vs %#x)" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ----------------------------------------------------------------------------- the definition: the per-op sequence

def per_op(rt, value, energy, region, mode, visualize):
    """include/silent_hip.h, silent_attention_tail: every call an existing entry point; advances ``energy``."""
    rh, rw = region
    dist, tot = rt.centroids(rt.affine_clip(value, div=255.0), rh, rw)
    imp = rt.affine_clip(tot, 255 / 4.0, 0.0, 1.0, 256.0, -1.0)
    ext = value.extents if isinstance(value, rt.PackedPyramid) else [tuple(value.shape[1:3])]
    half = [(int(np.float32(h) / th.DIV), int(np.float32(w) / th.DIV)) for h, w in ext]
    im2 = rt.resize_nearest(value, half if isinstance(value, rt.PackedPyramid) else half[0])
    dist2, _ = rt.centroids(rt.affine_clip(im2, div=255.0), rh, rw)
    fired, upd = rt.boosting_step(imp, energy, 1.0, 1.0, mode, visualize)
    return rt.affine_clip(dist, -255.0, 255.0), rt.affine_clip(dist2, -255.0, 255.0), rt.affine_clip(fired, 255.0), upd


def new_state(rt, extents, region, n_frames, fill=8.0):
    import torch
    cells = [(-(-h // region[0]), -(-w // region[1])) for h, w in extents]
    data = torch.full((n_frames * sum(h * w for h, w in cells),), fill, dtype=torch.float32, device="cuda:0")
    return rt.PackedPyramid(data, cells, 1, n_frames)


_VALUES = {}


def value_maps(rt, kernels, name, n_frames, n_calls=5):
    """kind -> n_calls packed 1-channel value maps of the geometry on the GPU: the chain's own output on structured frames (black
    background: many empty cells, and NaN where the regulator divides 0 by 0), noise in [0, 255], all zero.  Built once."""
    import torch
    key = (name, n_frames)
    if key not in _VALUES:
        ext = th.GEOMETRIES[name]
        ks = {k: kernels[k] for k in ("rgc", "rgby", "stripe", "blur", "end")}
        out = {"chain": [], "noise": [], "zero": []}
        for call in range(n_calls):
            lv = [np.stack([structured_frame(100 * call + 10 * f + l, h, w, 3, n_lines=max(3, h * w // 80)) for f in range(n_frames)])
                  for l, (h, w) in enumerate(ext)]
            x = rt.PackedPyramid.from_levels(lv)
            x = rt.PackedPyramid(torch.from_numpy(x.data).cuda(0), ext, 3, n_frames)
            out["chain"].append(rt.rgb_line_end(x, ks, want=("value",))["value"])
            nz = [np.stack([noise_frame(7000 + 100 * call + 10 * f + l, h, w, 1) for f in range(n_frames)]) for l, (h, w) in enumerate(ext)]
            out["noise"].append(rt.PackedPyramid(torch.from_numpy(rt.PackedPyramid.from_levels(nz).data).cuda(0), ext, 1, n_frames))
            out["zero"].append(rt.PackedPyramid(torch.zeros(n_frames * sum(h * w for h, w in ext), device="cuda:0"), ext, 1, n_frames))
        _VALUES[key] = out
    return _VALUES[key]


def test_the_chain_maps_hold_empty_cells_and_the_noise_maps_none(rt, kernels):
    """What the value kinds are for: NaN centroids on the chain's output, none on noise, all of them on the zero map."""
    v = value_maps(rt, kernels, "B", 3)
    nan = {}
    for kind in ("chain", "noise", "zero"):
        c1, c2, _, _ = rt.attention_tail(v[kind][0], new_state(rt, th.GEOMETRIES["B"], (3, 3), 3))
        nan[kind] = float(np.isnan(c1.data.cpu().numpy()).mean())
    print("share of NaN centroids:", nan)
    assert nan["chain"] > 0.0 and nan["noise"] == 0.0 and nan["zero"] == 1.0, nan


@pytest.mark.parametrize("region", th.REGIONS, ids=["%dx%d" % r for r in th.REGIONS])
@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("name", sorted(th.GEOMETRIES))
def test_fused_equals_per_op_bit_for_bit(rt, kernels, name, n_frames, region):
    """Five successive calls, the state carried on both sides: the four results and the state after every call, as uint32."""
    ext = th.GEOMETRIES[name]
    values = value_maps(rt, kernels, name, n_frames)
    for kind in ("chain", "noise", "zero"):
        for visualize in (0, 1):
            for mode in (CONSTANT, INPUT, CONSTANT | INPUT):
                a, b = new_state(rt, ext, region, n_frames), new_state(rt, ext, region, n_frames)
                for call, value in enumerate(values[kind]):
                    got = rt.attention_tail(value, a, region, recovery_mode=mode, visualize=bool(visualize))
                    want = per_op(rt, value, b, region, mode, bool(visualize))
                    what = "%s %s x%d region %s visualize %d mode %d call %d" % (name, kind, n_frames, region, visualize, mode, call)
                    for n, g, w in zip(RESULTS, got, want):
                        assert g.extents == w.extents and g.channels == w.channels, (what, n)
                        same_bits(g, w, what + ": " + n)
                    same_bits(a, b, what + ": state")
                assert bool((a.data != 8.0).all()), "a cell of the state never moved"      # (NaN != 8 too: a NaN value map makes NaN cells)


@pytest.mark.parametrize("name", sorted(th.GEOMETRIES))
def test_outputs_that_are_not_asked_for(rt, kernels, name):
    """centroids2_out = NULL, and only energy non-NULL: the remaining results and the state are those of the full call."""
    ext, region = th.GEOMETRIES[name], (3, 3)
    value = value_maps(rt, kernels, name, 3)["chain"][0]
    states = [new_state(rt, ext, region, 3) for _ in range(3)]
    full = rt.attention_tail(value, states[0])
    part = rt.attention_tail(value, states[1], want=("centroids", "fired", "update"))
    none = rt.attention_tail(value, states[2], want=())
    assert part[1] is None and none == (None, None, None, None)
    for i in (0, 2, 3):
        same_bits(part[i], full[i], "%s without centroids2: %s" % (name, RESULTS[i]))
    same_bits(states[1], states[0], name + " without centroids2: state")
    same_bits(states[2], states[0], name + " with only the state: state")


def test_the_host_form_and_the_nhwc_form_give_the_bits_of_the_device_form(rt, kernels):
    for name in sorted(th.GEOMETRIES):
        ext = th.GEOMETRIES[name]
        value = value_maps(rt, kernels, name, 3)["chain"][1]
        dev_state = new_state(rt, ext, (2, 3), 3)
        host_state = rt.PackedPyramid(np.full(dev_state.data.shape[0], 8, np.float32), dev_state.extents, 1, 3)
        host_value = rt.PackedPyramid(value.data.cpu().numpy(), ext, 1, 3)
        for call in range(2):
            got = rt.attention_tail(host_value, host_state, (2, 3), recovery_mode=INPUT)
            want = rt.attention_tail(value, dev_state, (2, 3), recovery_mode=INPUT)
            for n, g, w in zip(RESULTS, got, want):
                assert isinstance(g.data, np.ndarray)
                same_bits(g, w, "%s host form call %d: %s" % (name, call, n))
            same_bits(host_state, dev_state, "%s host form call %d: state" % (name, call))
    # an NHWC tensor: one level, results as tensors
    import torch
    x = torch.from_numpy(np.stack([noise_frame(5 + f, 37, 53, 1) for f in range(2)])).cuda(0)
    e1, e2 = torch.full((2, 13, 18, 1), 8.0, device="cuda:0"), torch.full((2, 13, 18, 1), 8.0, device="cuda:0")
    got, want = rt.attention_tail(x, e1), per_op(rt, x, e2, (3, 3), CONSTANT, True)
    assert [tuple(g.shape) for g in got] == [(2, 37, 53, 1), (2, 22, 32, 1), (2, 13, 18, 3), (2, 13, 18, 3)]
    for n, g, w in zip(RESULTS, got, want):
        same_bits(g, w, "NHWC: " + n)
    same_bits(e1, e2, "NHWC: state")
    with pytest.raises(ValueError, match="one value per centroid cell"):
        rt.attention_tail(x, torch.full((2, 13, 17, 1), 8.0, device="cuda:0"))


# ----------------------------------------------------------------------------- the CPU oracle

def test_against_the_cpu_oracle_on_geometry_a(rt):
    """oracle.line_end_displayer_tail on a padded line-end map, three successive steps of three streams: the comparisons and scales of
    test_line_end_displayer_three_frames (tests/test_gpu_parity.py); the fired mask exact."""
    import torch
    ext, n = th.GEOMETRIES["A"], 3
    (h, w), L = ext[0], len(ext)
    state = new_state(rt, ext, (3, 3), n)
    want_state = np.full((n * L, 6, 8, 1), 8, np.float32)
    for step in range(3):
        padded = np.stack([noise_frame(300 + 10 * step + i, h, w, 3) for i in range(n * L)])       # [frame-major (frame, level), h, w, 3]
        padded[:, :2] = padded[:, -2:] = 0
        padded[:, :, :2] = padded[:, :, -2:] = 0                                                    # pad_inwards(.., 2)
        padded[0, 4:10, 6:15] = 0                                                                   # empty cells: NaN centroids
        value = rt.PackedPyramid(rt.value_from_color(torch.from_numpy(padded).cuda(0)).reshape(-1), ext, 1, n)
        got = rt.attention_tail(value, state)
        tail, want_state = oracle.line_end_displayer_tail(padded, want_state)
        shapes = [(h, w, 1), (9, 14, 1), (6, 8, 3), (6, 8, 3)]
        for i, (name, g) in enumerate(zip(RESULTS, got)):
            g = g.data.cpu().numpy().reshape((n * L,) + shapes[i])
            assert g.shape == tail[i].shape, name
            scale = 255.0 * (h + w) if i < 2 else 255.0                # 255 - |c - x| * 255: pixel coordinates (< h + w) times 255
            assert_close(g, tail[i], RTOL, scale=scale, what="%s, step %d" % (name, step))
            if name == "fired":
                assert np.array_equal(g != 0, tail[i] != 0), "fired mask, step %d" % step
        assert np.isnan(tail[0]).any()
        assert_close(state.data.cpu().numpy().reshape(want_state.shape), want_state, RTOL, what="state, step %d" % step)


# ----------------------------------------------------------------------------- the pipeline

HW = (150, 230)
LAYOUTS = {"classic": dict(n_levels=3), "center_dimensions": dict(center_dimensions=(96, 64))}


def frames_of(step, slots, hw=HW):
    return np.stack([structured_frame(40 + 7 * step + s, hw[0], hw[1], 3) for s in slots])


def pipe(batch=3, layout="classic", **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    return LineEndPipeline(HW, mode="rgb", batch=batch, device=0, **dict(LAYOUTS[layout], **kw))


def tail_of(p, frame=None):
    """The four results and the state of a pipeline as arrays ([batch, ...] rows; ``frame``: that row)."""
    import torch
    torch.cuda.synchronize()
    out = p.outputs()
    rows = [out[n].data.reshape(p.batch, -1).cpu().numpy() for n in RESULTS] + [p.get_state()]
    return rows if frame is None else [r[frame] for r in rows]


def test_slots_are_streams(rt):
    import torch
    slots, perm = [0, 1, 2], [2, 0, 1]
    three, permuted, singles = pipe(attention=True), pipe(attention=True), [pipe(batch=1, attention=True) for _ in slots]
    assert three.energy.shape == (3, three.cells_per_frame) and float(three.energy.min()) == float(three.energy.max()) == 8.0
    for step in range(3):
        three.step(torch.from_numpy(frames_of(step, slots)).cuda(0))
        permuted.step(torch.from_numpy(frames_of(step, perm)).cuda(0))
        got, got_perm = tail_of(three), tail_of(permuted)
        for s in slots:
            singles[s].step(torch.from_numpy(frames_of(step, [s])).cuda(0))
            for n, a, b in zip(RESULTS + ("state",), [g[s] for g in got], tail_of(singles[s], 0)):
                same_bits(a, b, "step %d slot %d against a batch of one: %s" % (step, s, n))
        for i, s in enumerate(perm):
            for n, a, b in zip(RESULTS + ("state",), got_perm, got):
                same_bits(a[i], b[s], "step %d: permuted slot %d = slot %d: %s" % (step, i, s, n))
    before = three.get_state()
    assert before.shape == (3, three.cells_per_frame) and (before != 8.0).any(axis=1).all()
    three.set_state(three.get_state())
    same_bits(three.get_state(), before, "set_state(get_state())")
    three.reset_state([1])
    after = three.get_state()
    same_bits(after[[0, 2]], before[[0, 2]], "reset_state([1]): the other slots")
    assert (after[1] == 8.0).all()
    three.reset_state()
    assert (three.get_state() == 8.0).all()
    with pytest.raises(ValueError):
        three.set_state(before[:2])
    with pytest.raises(ValueError):
        three.reset_state([3])
    with pytest.raises(ValueError, match="attention"):
        pipe().get_state()


@pytest.mark.parametrize("entry", ["step", "step_host"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_tail_changes_nothing_else(rt, layout, entry):
    """Every other output and the keypoints of attention=True are those of attention=False on the same frames, bit for bit; and the
    tail's results are the per-op sequence on the pipeline's own value map."""
    import torch
    on, off = pipe(2, layout, attention=True, selection=True), pipe(2, layout, selection=True)
    ref_state = new_state(rt, on.extents, (3, 3), 2)
    for step in range(2):
        frames = frames_of(step, [0, 1])
        for p in (on, off):
            p.step_host(frames) if entry == "step_host" else p.step(torch.from_numpy(frames).cuda(0))
        torch.cuda.synchronize()
        a, b = on.outputs(), off.outputs()
        assert sorted(set(a) - set(b)) == sorted(RESULTS) and not set(b) - set(a)
        for k in sorted(b):
            if k == "keypoints":
                for f in range(2):
                    assert np.array_equal(a[k][f], b[k][f]), "keypoints of frame %d, step %d" % (f, step)
            elif k == "keypoint_counts":
                assert np.array_equal(a[k], b[k])
            else:
                same_bits(a[k], b[k], "%s %s step %d: %s" % (layout, entry, step, k))
        want = per_op(rt, a["value"], ref_state, (3, 3), CONSTANT, True)
        for n, w in zip(RESULTS, want):
            assert a[n].extents == w.extents and a[n].channels == w.channels
            same_bits(a[n], w, "%s %s step %d: %s against the per-op sequence" % (layout, entry, step, n))
        same_bits(on.energy, ref_state, "state")
    assert on.algorithmic_bytes_per_frame() - off.algorithmic_bytes_per_frame() == on.attention_bytes_per_frame() > 8 * on.frame_px
    assert "attn_cells_kernel" in on.launch_summary() and "attn_" not in off.launch_summary()


def test_the_reference_layout_gives_the_displayers_results(rt):
    """On the reference layout the four results are outputs 1 - 4 of LineEndDisplayer(native=False).run_device on the pipeline's own
    pyramid levels -- one displayer per frame slot (its state is one stream's), three steps."""
    import torch
    from pysilent_amd.recognition_testing import LineEndDisplayer
    p = pipe(2, "center_dimensions", attention=True)
    disp = [LineEndDisplayer(output_size=(96, 64), native=False) for _ in range(2)]
    assert len(set(p.extents)) == 1 and p.extents[0] == (64, 96)
    for step in range(3):
        p.step(torch.from_numpy(frames_of(step, [0, 1])).cuda(0))
        torch.cuda.synchronize()
        out = p.outputs()
        for f in range(2):
            pyr = torch.stack([lv[f] for lv in out["pyramid"].levels()])
            want = disp[f].run_device(pyr)
            for i, n in enumerate(RESULTS):
                got = torch.stack([lv[f] for lv in out[n].levels()])
                assert tuple(got.shape) == tuple(want[1 + i].shape), n
                same_bits(got, want[1 + i], "step %d frame %d: %s" % (step, f, n))
            same_bits(p.energy[f], disp[f].energy_values, "step %d frame %d: state" % (step, f))


def test_the_tuners_do_not_advance_a_stream(rt):
    """placement="auto" tunes on the first step: its timed steps leave the state alone, so state and results after that step are those
    of a placement=None pipeline after its first step; tune_placement called later leaves the state untouched bit for bit; tune_overlap
    is refused."""
    import torch
    frames = torch.from_numpy(frames_of(0, [0, 1, 2])).cuda(0)
    auto, plain = pipe(attention=True, placement="auto"), pipe(attention=True)
    auto.step(frames)
    plain.step(frames)
    assert auto.placement_tuning is not None and len(auto.placement_tuning["tries_ms"]) >= 1 and plain.placement_tuning is None
    for n, a, b in zip(RESULTS + ("state",), tail_of(auto), tail_of(plain)):
        same_bits(a, b, "after the first step: " + n)
    before = plain.get_state()
    plain.tune_placement(frames, tries=2, steps=2, budget_s=0.5)
    same_bits(plain.get_state(), before, "tune_placement")
    assert plain._attention_state is plain.energy
    with pytest.raises(ValueError, match="attention"):
        plain.tune_overlap()
    plain.step(frames)
    auto.step(frames)
    for n, a, b in zip(RESULTS + ("state",), tail_of(auto), tail_of(plain)):
        same_bits(a, b, "after the second step: " + n)


# ----------------------------------------------------------------------------- write coverage and stream order

WANTS = (RESULTS, ("centroids", "fired", "update"), ("fired",))


def _attn_calls(rt, x):
    """One call per output set; the state lies between guards of its own: it is an output too (updated in place)."""
    def call(want):
        def run():
            cells, _, _ = rt.attention_extents(x.extents, rt.attention_params())
            state = wc.result_like(x.data, (x.n_frames * sum(h * w for h, w in cells),))
            if hasattr(state, "fill_"):
                state.fill_(8.0)
            else:
                state[...] = 8
            res = rt.attention_tail(x, rt.PackedPyramid(state, cells, 1, x.n_frames), recovery_mode=CONSTANT | INPUT, want=want)
            return tuple(r for r in res if r is not None) + (state,)
        return run
    return [call(w) for w in WANTS]


def _attn_inputs():
    xs = [wcc.Packed([wcc.noise((2, h, w, 1), 8100 + i) for i, (h, w) in enumerate(th.GEOMETRIES[g])]) for g in ("B", "C")]
    for x in xs:
        x.data[np.random.default_rng(81).random(x.data.shape) > 0.4] = 0.0        # empty cells
    return xs


_PX = 2 * max(sum(h * w for h, w in th.GEOMETRIES[g]) for g in ("B", "C"))
CASE = wcc.Case("attention_tail", wcc.each(_attn_calls), _attn_inputs, _PX * 4 * 10, workspace=True)
# tests/test_gpu_stream_order.py finds every silent_*_dev with a host-memory argument by its signature and asks for a case that reaches
# it: silent_attention_tail_dev takes a silent_extent table.  The case is named here, when the suite is collected.
tso.HOST_ARG_CASES[CASE.id] = CASE
tso.REACHED_BY["attention_tail"] = CASE.id


def test_device_form_writes_all_and_only_its_output(rt, monkeypatch):
    tg.test_device_form_writes_all_and_only_its_output(rt, monkeypatch, CASE)


def test_host_form_does_not_return_stale_arena_bytes(rt):
    tg.test_host_form_does_not_return_stale_arena_bytes(rt, CASE)


def test_results_do_not_depend_on_the_previous_call(rt):
    tg.test_results_do_not_depend_on_the_previous_call(rt, CASE)


@pytest.fixture(scope="module")
def h(rt):
    return so.Harness(rt)


def test_calls_behind_a_producer_and_before_an_overwriter(rt, h):
    """Every call on a held stream of the caller's, behind the producer of ``value`` and in front of an overwriter: the bits of the
    quiet call, returned while the hold is pending, on torch's current stream, given the value buffer itself."""
    subj = so.subject(CASE)
    bufs = so.Buffers(rt, subj, subj.decoy)
    assert len(bufs.calls) == 2 * len(WANTS)
    with h.watching() as w:
        bufs.calls[0]()
    assert [r["name"] for r in w.records] == ["silent_attention_tail_dev"]
    for i in range(len(bufs.calls)):
        so.scenario_producer_call_overwriter(h, subj, i, bufs)


def test_two_streams_and_the_host_form_behind_a_device_form(rt, h):
    subj = so.subject(CASE)
    pair = so.Buffers(rt, subj, subj.a), so.Buffers(rt, subj, subj.b)
    so.scenario_two_streams(h, subj, 0, pair)
    so.scenario_two_streams(h, subj, 0, pair, hold_both=True)
    host_calls = subj.calls(rt, *[wcc.on_host(rt, v) for v in subj.b])
    so.scenario_host_form_behind_device_form(h, subj, 0, pair[0], host_calls)
