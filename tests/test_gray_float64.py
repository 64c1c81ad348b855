"""Float64 accumulation of the gray pass on the GPU (SILENT_PLAN_ACCUM_F64; PyramidPlan / LineEndPipeline(accumulation="float64")).
Every op sums its taps in float64 and rounds once to float32, like the C oracle: the pyramid is within 1 ulp of the oracle's 2-D
float64 sum (and bit-identical on the reference's own goldens), the CS and end maps of a given pyramid are bit-identical to the
oracle's, so the maps from a frame meet the 1e-5 contract element by element and the keypoints equal the oracle chain's.
These criteria are asserted directly here; nothing goes through conftest.assert_close."""
import math

import numpy as np
import pytest

from conftest import noise_frame, structured_frame

pytestmark = pytest.mark.gpu

E5 = float(math.e) ** .5


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _ordered(a):
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def _canon_bits(a):
    """int32 patterns with every NaN mapped to one pattern (a NaN's sign and payload are not part of the contract)."""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _nonfinite_frame(seed, h, w):
    f = noise_frame(seed, h, w, 1).copy()
    rng = np.random.default_rng(1000 + seed)
    for v in (np.nan, np.inf, -np.inf):
        ys, xs = rng.integers(0, h, 6), rng.integers(0, w, 6)
        f[ys, xs, 0] = v
    return f


def _levels(name):
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    if name in ("config2", "config2_nostream"):
        return (1080, 1920), classic_levels((1080, 1920), 2.0, 5)
    if name == "config5":
        return (2160, 3840), classic_levels((2160, 3840), 2.0, 8)
    if name == "sqrt2":
        return (540, 960), classic_levels((540, 960), 2.0 ** .5, 8)
    if name == "reference_crop":
        return (1080, 1920), reference_levels((1080, 1920), (288, 192), E5)
    if name == "config1":
        return (480, 640), classic_levels((480, 640), 2.0, 3)
    raise KeyError(name)


class _Knobs(object):
    """config2_nostream: the stream path switched off (SILENT_TUNE_GRAY bit 4; silent_pyramid: SILENT_TUNE_PYRAMID bit 0)."""

    def __init__(self, rt, name):
        self.rt, self.on = rt, name == "config2_nostream"

    def __enter__(self):
        from pysilent_amd import _lib
        if self.on:
            self.g = self.rt.tuning(_lib.TUNE_GRAY, 16)
            self.p = self.rt.tuning(_lib.TUNE_PYRAMID, 1)
            self.g.__enter__()
            self.p.__enter__()

    def __exit__(self, *exc):
        if self.on:
            self.p.__exit__(*exc)
            self.g.__exit__(*exc)


def _plan(rt, name):
    hw, levels = _levels(name)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0, accumulation="float64")
    assert plan.accumulation == "float64" and plan.flags == 1
    return hw, levels, plan


def _oracle_pyramid(frame, levels):
    import c_oracle as co
    return [co.zoom_level(frame, *l)[:, :, 0] for l in levels]


def _pyramid_ulps(got_levels, want_levels, levels):
    """(max ulps, elements not bit-identical, elements) over the resampled part of every level."""
    worst = differ = total = 0
    for g, w, l in zip(got_levels, want_levels, levels):
        d = np.abs(_ordered(g) - _ordered(w))
        worst = max(worst, int(d.max()))
        differ += int((d != 0).sum())
        total += d.size
    return worst, differ, total


PLANS = ["config2", "config5", "sqrt2", "reference_crop", "config2_nostream"]


@pytest.mark.parametrize("name", PLANS)
def test_pyramid_within_one_ulp_of_the_oracle(rt, name):
    hw, levels, plan = _plan(rt, name)
    if name == "sqrt2":
        assert plan.streamable   # (a dense ladder: slot layout 1 of the stream kernels)
    if name == "reference_crop":
        assert not plan.streamable
    frame = noise_frame(7, hw[0], hw[1], 1)
    with _Knobs(rt, name):
        pyr = plan.run(frame[None])
    got = [pyr.level(l)[0].reshape(h, w) for l, (h, w) in enumerate(plan.extents)]
    worst, differ, total = _pyramid_ulps(got, _oracle_pyramid(frame, levels), levels)
    print("%s pyramid: max %d ulp, %d of %d elements not bit-identical (share %.2e)" % (name, worst, differ, total, differ / total))
    assert worst <= 1 and differ <= 1e-5 * total
    plan.close()


@pytest.mark.parametrize("case", ["gray_three", "nonfinite_gray"])
def test_pyramid_bit_identical_on_the_reference_goldens(rt, golden_pyramid, case):
    from pysilent_amd.util.zoom.from_image import reference_levels
    img, want, par = golden_pyramid[case]
    center, scale = [int(par[0]), int(par[1])], float(par[2])
    levels = reference_levels(img.shape[:2], center, scale)
    plan = rt.PyramidPlan(img.shape[0], img.shape[1], 1, levels, 0, accumulation="float64")
    packed = plan.run(np.ascontiguousarray(img[None], np.float32))
    h, w = packed.extents[0]
    got = np.asarray(packed.data).reshape(len(levels), h, w, 1)
    want = want.astype(np.float32)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    assert np.array_equal(_canon_bits(got), _canon_bits(want)), "%s: %d elements differ" % (
        case, int((_canon_bits(got) != _canon_bits(want)).sum()))
    plan.close()


def _gray_pass(rt, plan, frames, K, cs_only=False):
    """silent_gray_pass (host form) of an F64 plan; cs_only: end_out = NULL (config 1)."""
    from pysilent_amd import _lib
    from pysilent_amd.pipeline import default_constants
    consts = default_constants("gray", K)
    cs_k, end_k = np.ascontiguousarray(consts["cs"], np.float32), np.ascontiguousarray(consts["end"], np.float32)
    n, px = frames.shape[0], plan.frame_px
    pyr, cs = np.zeros(n * px, np.float32), np.zeros(n * px, np.float32)
    end = None if cs_only else np.zeros(n * px * K, np.float32)
    frames = np.ascontiguousarray(frames, np.float32)
    plan.ctx.check(_lib.load().silent_gray_pass(plan.ctx.handle, plan.handle, frames.ctypes.data, n, cs_k.ctypes.data,
                                                end_k.ctypes.data, K, 255.0, pyr.ctypes.data, cs.ctypes.data,
                                                None if end is None else end.ctypes.data))
    P = rt.PackedPyramid
    return P(pyr, plan.extents, 1, n), P(cs, plan.extents, 1, n), (None if end is None else P(end, plan.extents, K, n)), cs_k, end_k


@pytest.mark.parametrize("name", PLANS + ["config1"])
def test_cs_and_end_bit_identical_to_the_oracle_on_the_gpu_pyramid(rt, name):
    import c_oracle as co
    hw, levels, plan = _plan(rt, name)
    if name == "config5":
        frames = np.stack([structured_frame(3, hw[0], hw[1], 1), _nonfinite_frame(4, hw[0], hw[1])])
    else:
        frames = np.stack([noise_frame(1, hw[0], hw[1], 1), structured_frame(2, hw[0], hw[1], 1), _nonfinite_frame(3, hw[0], hw[1])])
    for K in ((4,) if name == "config1" else (3, 4, 8)):
        with _Knobs(rt, name):
            pyr, cs, end, cs_k, end_k = _gray_pass(rt, plan, frames, K, cs_only=name == "config1")
        worst = 0
        for f in range(len(frames)):
            for l, (h, w) in enumerate(plan.extents):
                lev = np.ascontiguousarray(pyr.level(l)[f].reshape(h, w))
                want_cs, want_end = co.gray_line_end_level(lev[None, :, :, None], cs_k, end_k, 255.0)
                got_cs = cs.level(l)[f].reshape(h, w)
                assert np.array_equal(_canon_bits(got_cs), _canon_bits(want_cs[0, :, :, 0])), \
                    "%s K=%d frame %d level %d: CS differs" % (name, K, f, l)
                if end is not None:
                    got_end = end.level(l)[f].reshape(h, w, K)
                    assert np.array_equal(_canon_bits(got_end), _canon_bits(want_end[0])), \
                        "%s K=%d frame %d level %d: end differs" % (name, K, f, l)
                if K == 4 and np.isfinite(frames[f]).all():   # (finite frames: this pyramid is within 1 ulp of the oracle too)
                    d = np.abs(_ordered(lev) - _ordered(_oracle_pyramid(frames[f], [levels[l]])[0]))
                    worst = max(worst, int(d.max()))
        assert worst <= 1, "%s K=%d: gray_pass pyramid %d ulps from the oracle" % (name, K, worst)
    plan.close()


def _contract(rt, name, frames, K):
    """Shares of the 1e-5 contract on the maps from the frame: (checked elements out of tolerance, excluded share)."""
    import c_oracle as co
    from scipy.ndimage import binary_dilation
    hw, levels, plan = _plan(rt, name)
    pyr, cs, end, cs_k, end_k = _gray_pass(rt, plan, frames, K)
    checked = bad = excluded = total = 0
    for f in range(len(frames)):
        want_pyr = _oracle_pyramid(frames[f], levels)
        maps = []
        for l, (h, w) in enumerate(plan.extents):
            diff = pyr.level(l)[f].reshape(h, w) != want_pyr[l]
            wc, we = co.gray_line_end_level(want_pyr[l][None, :, :, None], cs_k, end_k, 255.0)
            maps.append((diff, cs.level(l)[f].reshape(h, w), wc[0, :, :, 0], end.level(l)[f].reshape(h, w, K), we[0]))
        for kind, r in (("cs", 1), ("end", 2)):
            wants = [m[2] if kind == "cs" else m[4] for m in maps]
            rng = max(float(np.nanmax(w)) - float(np.nanmin(w)) for w in wants)
            for diff, gcs, wcs, gend, wend in maps:
                got, want = (gcs, wcs) if kind == "cs" else (gend, wend)
                ex = binary_dilation(diff, structure=np.ones((2 * r + 1, 2 * r + 1), bool))
                if kind == "end":
                    ex = ex[:, :, None].repeat(K, axis=2)
                sel = (np.abs(want) >= 1e-3 * rng) & ~ex
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.abs(got.astype(np.float64) - want) / np.abs(want)
                checked += int(sel.sum())
                bad += int((rel[sel] > 1e-5).sum())
                excluded += int(ex.sum())
                total += ex.size
    plan.close()
    return checked, bad, excluded, total


@pytest.mark.parametrize("name,K,n", [("config2", 4, 2), ("config5", 8, 1)])
def test_maps_from_the_frame_meet_the_1e5_contract(rt, name, K, n):
    hw, _ = _levels(name)
    frames = np.stack([(noise_frame if i % 2 == 0 else structured_frame)(20 + i, hw[0], hw[1], 1) for i in range(n)])
    checked, bad, excluded, total = _contract(rt, name, frames, K)
    print("%s float64: %d of %d checked CS/end elements beyond 1e-5 (share %.2e); excluded share %.2e "
          "(the float32 path: 1.5 %% / 10 %% beyond)" % (name, bad, checked, bad / max(checked, 1), excluded / total))
    assert checked > 0 and bad == 0
    assert excluded <= 1e-5 * total


def _gray_pipe(hw, K, batch, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    return LineEndPipeline(hw, mode="gray", n_orient=K, batch=batch, device=0, **kw)


@pytest.mark.parametrize("selection", [True, False])
def test_keypoints_equal_the_oracle_chain(rt, selection):
    import torch
    import c_oracle as co
    from gray_kp_oracle import gray_tail
    hw, K, n_levels = (360, 640), 4, 4
    frames = np.stack([noise_frame(31, hw[0], hw[1], 1), structured_frame(32, hw[0], hw[1], 1)])
    pipe = _gray_pipe(hw, K, 2, n_levels=n_levels, keypoints=True, selection=selection, accumulation="float64")
    assert pipe.accumulation == "float64" and "float64" in pipe.launch_summary()
    pipe.step(torch.from_numpy(frames).cuda(0))
    out = pipe.outputs()
    cs_k, end_k = pipe.consts["cs"], pipe.consts["end"]
    levels = pipe.plan.levels
    for f in range(2):
        gpu_pyr = [out["pyramid"].level(l)[f].cpu().numpy().reshape(h, w) for l, (h, w) in enumerate(pipe.extents)]
        # (a) the oracle's tail on the oracle's end maps of the GPU's own pyramid
        ends = [co.gray_line_end_level(p[None, :, :, None], cs_k, end_k, pipe.clip_hi)[1][0] for p in gpu_pyr]
        rows, _, _ = gray_tail(ends, pad=pipe.pad, selection=selection, top_percent=pipe.top_percent)
        assert int(out["keypoint_counts"][f]) == len(rows)
        assert np.array_equal(out["keypoints"][f], rows), "frame %d: rows differ from the oracle tail" % f
        # (b) the oracle's whole chain from the frame: its pyramid first, bit for bit
        want_pyr = _oracle_pyramid(frames[f], levels)
        for l in range(len(levels)):
            assert np.array_equal(_canon_bits(gpu_pyr[l]), _canon_bits(want_pyr[l])), "frame %d level %d: pyramid" % (f, l)
        ends = [co.gray_line_end_level(p[None, :, :, None], cs_k, end_k, pipe.clip_hi)[1][0] for p in want_pyr]
        rows, _, _ = gray_tail(ends, pad=pipe.pad, selection=selection, top_percent=pipe.top_percent)
        assert np.array_equal(out["keypoints"][f], rows), "frame %d: rows differ from the oracle chain" % f


def _maps(out):
    return {k: out[k].data.clone() for k in ("pyramid", "cs", "end")}


def _same_maps(a, b):
    import torch
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_overlap_step_host_and_default_paths_agree(rt):
    import torch
    hw, K, batch = (540, 960), 4, 2
    u8 = np.stack([np.random.default_rng(40 + i).integers(0, 256, (hw[0], hw[1], 1)).astype(np.uint8) for i in range(batch)])
    f32 = torch.from_numpy(u8.astype(np.float32)).cuda(0)
    base = _gray_pipe(hw, K, batch, accumulation="float64")
    base.step(f32)
    want = _maps(base.outputs())
    ov = _gray_pipe(hw, K, batch, accumulation="float64", overlap="force")
    ov.step(f32)
    ov.step(f32)
    assert _same_maps(_maps(ov.outputs()), want), "overlap='force' differs from step"
    host = _gray_pipe(hw, K, batch, accumulation="float64")
    host.step_host(u8)
    assert _same_maps(_maps(host.outputs()), want), "step_host (uint8) differs from step"
    tuned = _gray_pipe(hw, K, batch, accumulation="float64", placement="auto")
    tuned.step(f32)
    assert _same_maps(_maps(tuned.outputs()), want), "the placement tuner changed the float64 maps"
    a = _gray_pipe(hw, K, batch)
    a.step(f32)
    b = _gray_pipe(hw, K, batch, accumulation="float32")
    b.step(f32)
    assert a.accumulation == "float32" and a.launch_summary() == b.launch_summary()
    assert _same_maps(_maps(a.outputs()), _maps(b.outputs())), "accumulation='float32' differs from the default"
    for p in (base, ov, host, tuned, a, b):
        p.close()
