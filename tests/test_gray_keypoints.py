"""LineEndPipeline(mode="gray", keypoints=True) / silent_gray_keypoints_dev on the GPU: the maps are those of the maps-only
step, the keypoints, counts and value maps are those of the GPU per-op composite on the same end map (pad_inwards ->
top_value_points -> nms3x3 -> value_from_color -> max_value_indices_region), bit for bit, and the oracle's tail on the
downloaded end map gives the same rows."""
import math

import numpy as np
import pytest

from conftest import noise_frame, structured_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return bool(torch.equal(_bits(a), _bits(b)))


def _pipe(hw, K, batch, keypoints, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    return LineEndPipeline(hw, mode="gray", n_orient=K, batch=batch, device=0, keypoints=keypoints, **kw)


def _frames(hw, batch, seed=0, kind="mixed"):
    import torch
    fs = [(structured_frame(seed + i, hw[0], hw[1], 1) if (kind == "structured" or (kind == "mixed" and i % 2)) else
           noise_frame(seed + i, hw[0], hw[1], 1)) for i in range(batch)]
    return torch.from_numpy(np.stack(fs)).cuda(0)


def _composite(rt, out, pad, selection, top_percent, regions):
    """The GPU per-op path on the pipeline's own end map."""
    end = out["end"]
    color = rt.pad_inwards(end, pad, pad, pad, pad)
    value = rt.value_from_color(color)
    v = value
    if selection:
        v = rt.value_from_color(rt.nms3x3(rt.top_value_points(color, top_percent, value)))
    idx, counts = rt.max_value_indices_region(v, regions)
    return value, v, idx, counts


def _check_against_composite(rt, pipe, out, selection, top_percent):
    import torch
    torch.cuda.synchronize()
    regions = [(pipe.regions[l].h, pipe.regions[l].w) for l in range(pipe.n_levels)]
    value, pv, idx, counts = _composite(rt, out, pipe.pad, selection, top_percent, regions)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    assert np.array_equal(out["keypoint_counts"], counts), (out["keypoint_counts"], counts)
    for f in range(pipe.batch):
        want = idx[f, :counts[f]].cpu().numpy()
        assert np.array_equal(out["keypoints"][f], want), "frame %d: keypoints differ from the per-op composite" % f
    if "value" in out:
        assert _same(out["value"].data, value.data), "value map differs"
    if "peak_value" in out:
        assert _same(out["peak_value"].data, pv.data), "peak-value map differs"
    return counts


GEOMETRIES = [
    # (frame hw, K, batch, pipeline geometry)
    ((120, 160), 3, 3, dict(scale=2.0, n_levels=3)),
    ((97, 233), 4, 1, dict(scale=math.e ** .5, n_levels=4)),
    ((224 + 1, 448 + 3), 8, 2, dict(scale=2.0, n_levels=4)),             # tile boundaries: one row / column past a tile
    ((150, 200), 4, 8, dict(center_dimensions=(48, 32), scale=math.e ** .5)),   # the reference's centre-crop layout
    ((150, 200), 8, 3, dict(center_dimensions=(48, 32), scale=2.0)),
    ((9, 13), 4, 3, dict(scale=2.0, n_levels=2)),                        # tiny frames
]


@pytest.mark.parametrize("hw,K,batch,geo", GEOMETRIES)
def test_maps_bit_identical_to_the_maps_only_step(rt, hw, K, batch, geo):
    frames = _frames(hw, batch, seed=K)
    ref = _pipe(hw, K, batch, False, **geo)
    ref.step(frames)
    want = ref.outputs()
    for selection in (True, False):
        pipe = _pipe(hw, K, batch, True, selection=selection, value_map=True, **geo)
        pipe.step(frames)
        out = pipe.outputs()
        for k in ("pyramid", "cs", "end"):
            assert _same(out[k].data, want[k].data), "%s differs from the maps-only step (selection=%s)" % (k, selection)
        _check_against_composite(rt, pipe, out, selection, 0.1)


@pytest.mark.parametrize("K", [3, 4, 8])
@pytest.mark.parametrize("top_percent", [0.0, 0.1, 0.37, 1.0])
def test_keypoints_identical_to_the_gpu_composite(rt, K, top_percent):
    hw = (130, 210)
    frames = _frames(hw, 2, seed=11 + K)
    for selection in (True, False):
        pipe = _pipe(hw, K, 2, True, selection=selection, top_percent=top_percent, n_levels=3, value_map=True,
                     peak_value_map=selection)
        pipe.step(frames)
        out = pipe.outputs()
        _check_against_composite(rt, pipe, out, selection, top_percent)
        # the sparse-tail-free form (no peak-value map) gives the same rows
        if selection:
            bare = _pipe(hw, K, 2, True, selection=True, top_percent=top_percent, n_levels=3)
            bare.step(frames)
            o2 = bare.outputs()
            assert bare.sparse_tail_stats()["ran"]
            assert np.array_equal(o2["keypoint_counts"], out["keypoint_counts"])
            for f in range(2):
                assert np.array_equal(o2["keypoints"][f], out["keypoints"][f])


@pytest.mark.parametrize("selection", [True, False])
def test_oracle_tail_on_the_gpu_end_map(rt, selection):
    from gray_kp_oracle import gray_tail
    hw, K = (110, 170), 4
    frames = _frames(hw, 2, seed=5, kind="structured")
    pipe = _pipe(hw, K, 2, True, selection=selection, n_levels=3)
    pipe.step(frames)
    out = pipe.outputs()
    for f in range(2):
        ends = [out["end"].level(l)[f].cpu().numpy() for l in range(pipe.n_levels)]
        rows, _, _ = gray_tail(ends, pad=pipe.pad, selection=selection, top_percent=0.1)
        assert np.array_equal(out["keypoints"][f], rows), "frame %d: GPU rows differ from the oracle's tail" % f


def _sparse_vs_dense(rt, frames, hw, K, **kw):
    from pysilent_amd._lib import TUNE_GRAY
    outs = []
    for knob in (0, 64):
        with rt.tuning(TUNE_GRAY, knob):
            pipe = _pipe(hw, K, frames.shape[0], True, selection=True, **kw)
            pipe.step(frames)
            out = pipe.outputs()
            stats = pipe.sparse_tail_stats()
            assert stats["ran"] == (knob == 0)
            outs.append((out, stats))
            _check_against_composite(rt, pipe, out, True, 0.1)
    (a, stats), (b, _) = outs
    assert np.array_equal(a["keypoint_counts"], b["keypoint_counts"])
    for f in range(frames.shape[0]):
        assert np.array_equal(a["keypoints"][f], b["keypoints"][f])
    return stats


def test_nan_and_inf_frames_take_the_dense_route(rt):
    import torch
    hw, K = (96, 160), 4
    frames = _frames(hw, 3, seed=21).cpu().numpy()
    frames[0, 40:43, 50:52, 0] = np.nan
    frames[1, 10, 10, 0] = np.inf
    frames[1, 60, 100, 0] = -np.inf
    frames[2] = 0.0                                                    # black: every window without a positive peak
    frames = torch.from_numpy(frames).cuda(0)
    stats = _sparse_vs_dense(rt, frames, hw, K, n_levels=3, value_map=True, peak_value_map=True)
    assert stats["dense_pairs"] >= 1
    _sparse_vs_dense(rt, frames, hw, 8, n_levels=3)


def test_candidate_overflow_at_k8(rt):
    import torch
    h, w = 400, 640
    grid = np.zeros((h, w, 1), np.float32)
    grid[::4, ::4] = 255.0                                               # > 16384 identical dots: the frame goes dense
    frames = torch.from_numpy(np.stack([grid, noise_frame(43, h, w, 1)])).cuda(0)
    stats = _sparse_vs_dense(rt, frames, (h, w), 8, n_levels=2, top_percent=0.1)
    assert stats["candidates"] > 16384 and stats["dense_pairs"] >= 2


def test_overflow_raises_and_truncation_keeps_the_true_counts(rt):
    hw = (64, 96)
    frames = _frames(hw, 2, seed=3)
    full = _pipe(hw, 4, 2, True, selection=False, n_levels=2)
    full.step(frames)
    want = full.outputs()
    cap = int(want["keypoint_counts"].min()) // 2
    assert cap > 0
    pipe = _pipe(hw, 4, 2, True, selection=False, n_levels=2, max_keypoints_per_frame=cap)
    pipe.step(frames)
    with pytest.raises(ValueError, match="capacity"):
        pipe.outputs()
    out = pipe.outputs(allow_truncated=True)
    assert np.array_equal(out["keypoint_counts"], want["keypoint_counts"])
    for f in range(2):
        assert np.array_equal(out["keypoints"][f], want["keypoints"][f][:cap])


def test_overlap_is_refused_and_the_placement_tuner_works(rt):
    hw = (96, 128)
    with pytest.raises(ValueError, match="overlap"):
        _pipe(hw, 4, 2, True, overlap="force")
    frames = _frames(hw, 2, seed=8)
    plain = _pipe(hw, 4, 2, True, selection=True, n_levels=3)
    plain.step(frames)
    want = plain.outputs()
    tuned = _pipe(hw, 4, 2, True, selection=True, n_levels=3, placement="auto")
    tuned.step(frames)                                                   # the tuner runs on this first batch
    assert tuned.placement_tuning is not None
    out = tuned.outputs()
    for k in ("pyramid", "cs", "end"):
        assert _same(out[k].data, want[k].data)
    assert np.array_equal(out["keypoint_counts"], want["keypoint_counts"])
    for f in range(2):
        assert np.array_equal(out["keypoints"][f], want["keypoints"][f])


@pytest.mark.parametrize("hw,K,batch,n_levels", [((1080, 1920), 4, 2, 5), ((2160, 3840), 8, 1, 8)])
def test_full_size_against_the_composite(rt, hw, K, batch, n_levels):
    frames = _frames(hw, batch, seed=31)
    ref = _pipe(hw, K, batch, False, n_levels=n_levels)
    ref.step(frames)
    want = ref.outputs()
    for selection in (True, False):
        pipe = _pipe(hw, K, batch, True, selection=selection, n_levels=n_levels)
        pipe.step(frames)
        out = pipe.outputs()
        for k in ("pyramid", "cs", "end"):
            assert _same(out[k].data, want[k].data)
        _check_against_composite(rt, pipe, out, selection, 0.1)
