"""float16 storage of the gray pass's CS and end maps on the GPU (silent_gray_pass_h; PyramidPlan.gray_pass / LineEndPipeline with
storage="float16").  Contract: every stored element is float16(v), v being the float32 value the float32-storage path of the same
build stores there, rounded to nearest even (overflow to inf, NaN stays NaN, subnormals kept); the pyramid stays float32, bit for
bit.  So the maps are compared bit for bit with NumPy's cast of the float32 path's maps (NumPy casts round-to-nearest-even), and
against the oracle with the float32 path's own bound plus half a float16 ulp.  Nothing goes through conftest.assert_close."""
import math

import numpy as np
import pytest

import err_bound as eb
from conftest import noise_frame, structured_frame

pytestmark = pytest.mark.gpu

E5 = float(math.e) ** .5


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _half_bits(a):
    """uint16 patterns of a float16 array with every NaN mapped to one pattern (sign and payload are not part of the contract)."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float16
    b = a.view(np.uint16).copy()
    b[np.isnan(a)] = 0x7e00
    return b


def _cast_bits(f32):
    """What the float16 path must store for a float32 map: NumPy's cast (round-to-nearest-even, overflow to inf)."""
    with np.errstate(over="ignore"):
        return _half_bits(np.ascontiguousarray(f32, np.float32).astype(np.float16))


def _f32_bits(a):
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
    if name == "odd":            # odd widths on every level (CS rows on 2-byte boundaries, levels at odd pixel offsets), tiles cut by both edges
        return (135, 241), classic_levels((135, 241), 2.0, 3)
    raise KeyError(name)


class _Knobs(object):
    """config2_nostream: the stream path switched off (SILENT_TUNE_GRAY bit 4): region + unit-fused + filter kernels."""

    def __init__(self, rt, name):
        self.rt, self.on = rt, name == "config2_nostream"

    def __enter__(self):
        from pysilent_amd import _lib
        if self.on:
            self.g = self.rt.tuning(_lib.TUNE_GRAY, 16)
            self.g.__enter__()

    def __exit__(self, *exc):
        if self.on:
            self.g.__exit__(*exc)


def _consts(K):
    from pysilent_amd.pipeline import default_constants
    c = default_constants("gray", K)
    return np.ascontiguousarray(c["cs"], np.float32), np.ascontiguousarray(c["end"], np.float32)


def _pass32(plan, frames, K):
    cs_k, end_k = _consts(K)
    return plan.gray_pass(frames, cs_k, end_k, 255.0)


def _pass16(plan, frames, K, want_cs=True, want_end=True):
    """silent_gray_pass_h (host form); cs_out / end_out may be NULL."""
    from pysilent_amd import _lib
    cs_k, end_k = _consts(K)
    n, px = frames.shape[0], plan.frame_px
    pyr = np.full(n * px, -7.0, np.float32)
    cs = np.full(n * px, 0x5555, np.uint16) if want_cs else None
    end = np.full(n * px * K, 0x5555, np.uint16) if want_end else None
    frames = np.ascontiguousarray(frames, np.float32)
    plan.ctx.check(_lib.load().silent_gray_pass_h(
        plan.ctx.handle, plan.handle, frames.ctypes.data, n, cs_k.ctypes.data, end_k.ctypes.data, K, 255.0, pyr.ctypes.data,
        _lib.half_ptr(None if cs is None else cs.ctypes.data), _lib.half_ptr(None if end is None else end.ctypes.data)))
    return pyr, (None if cs is None else cs.view(np.float16)), (None if end is None else end.view(np.float16))


PLANS = ["config1", "config2", "config5", "sqrt2", "reference_crop", "config2_nostream", "odd"]


@pytest.mark.parametrize("name", PLANS)
def test_bit_identical_to_the_cast_of_the_float32_path(rt, name):
    """Every element of cs and end, every level, every frame of the batch: uint16 pattern == float16(float32 path's value)."""
    hw, levels = _levels(name)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    if name in ("sqrt2", "config2", "config5", "config1", "odd"):
        assert plan.streamable
    if name == "reference_crop":
        assert not plan.streamable
    if name in ("sqrt2", "odd"):
        assert any(w % 2 for _, w in plan.extents), "this plan is here for its odd-width levels"
    frames = np.stack([noise_frame(1, hw[0], hw[1], 1), structured_frame(2, hw[0], hw[1], 1), _nonfinite_frame(3, hw[0], hw[1])])
    if name == "config5":
        frames = frames[1:]           # (4K: a batch of two -- structured + non-finite; noise runs on every other plan)
    checked = 0
    for K in (3, 4, 8):
        with _Knobs(rt, name):
            p32, c32, e32 = _pass32(plan, frames, K)
            p16, c16, e16 = _pass16(plan, frames, K)
        assert np.array_equal(_f32_bits(p16), _f32_bits(p32.data)), "%s K=%d: the pyramid differs from the float32 path's" % (name, K)
        for what, got, want in (("cs", c16, c32.data), ("end", e16, e32.data)):
            assert got.size == want.size
            gb, wb = _half_bits(got), _cast_bits(want)
            bad = int((gb != wb).sum())
            if bad:
                i = int(np.flatnonzero(gb != wb)[0])
                raise AssertionError("%s K=%d %s: %d of %d elements differ; first at %d: got 0x%04x, float32 %r -> 0x%04x"
                                     % (name, K, what, bad, gb.size, i, gb[i], float(want[i]), wb[i]))
            checked += gb.size
        assert np.isnan(c32.data).any() and np.isnan(e32.data).any()     # the non-finite frame reaches both maps
    print("%s: %d elements bit-identical to float16(float32 path)" % (name, checked))
    plan.close()


def test_rounding_is_to_nearest_even_on_values_that_tell(rt):
    """The frames above must contain values whose float16 differs between round-to-nearest-even and truncation, ties included is
    not required -- but SOME stored value must round UP, or a truncating store would pass."""
    hw, levels = _levels("config1")
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    frames = noise_frame(5, hw[0], hw[1], 1)[None]
    _, c32, e32 = _pass32(plan, frames, 4)
    _, c16, e16 = _pass16(plan, frames, 4)
    for f32m, f16m in ((c32.data, c16), (e32.data, e16)):
        up = f16m.astype(np.float32) > f32m
        assert up.any() and (f16m.astype(np.float32) < f32m).any()
        rtz = (f32m.view(np.uint32) & 0xffffe000).view(np.float32).astype(np.float16)      # truncation towards zero
        assert (rtz.view(np.uint16) != f16m.view(np.uint16)).any()
    plan.close()


@pytest.mark.parametrize("name,K,kinds", [("config1", 4, "ns"), ("config2", 4, "ns"), ("odd", 3, "ns"), ("odd", 8, "ns")])
def test_against_the_oracle_within_the_float32_bound_plus_half_a_float16_ulp(rt, name, K, kinds):
    """|float(h) - oracle| <= B32 + max(2^-11 (|oracle| + B32), 2^-25) for EVERY element: B32 is the float32 path's rounding bound
    against the oracle (err_bound.zoom / gray_chain, propagated from the frame), so the float32 value lies within B32 of the
    oracle; its float16 is within half an ulp of it: 2^-11 relative in the normal range, 2^-25 absolute below 2^-14."""
    import c_oracle as co
    hw, levels = _levels(name)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    frames = np.stack([(noise_frame if k == "n" else structured_frame)(11 + i, hw[0], hw[1], 1) for i, k in enumerate(kinds)])
    cs_k, end_k = _consts(K)
    _, cs, end = plan.gray_pass(frames, cs_k, end_k, 255.0, storage="float16")
    assert cs.dtype == np.float16 and end.dtype == np.float16 and cs.data.dtype == np.float16
    total = 0
    for f in range(len(frames)):
        for l, lv in enumerate(levels):
            h, w = plan.extents[l]
            want_pyr = co.zoom_level(frames[f], *lv)[:, :, 0]
            want_cs, want_end = co.gray_line_end_level(want_pyr[None, :, :, None], cs_k, end_k, 255.0)
            e_cs, e_end = eb.gray_chain(want_pyr[None, :, :, None], cs_k, end_k, want_cs, eb.zoom(want_pyr[None, :, :, None]))
            for what, got, want, b32 in (("cs", cs.level(l)[f], want_cs[0], e_cs[0]), ("end", end.level(l)[f], want_end[0], e_end[0])):
                assert not eb.unbounded(b32).any()                 # finite frames: every element has a finite bound
                want = want.astype(np.float64)
                bound = b32 + np.maximum(2.0 ** -11 * (np.abs(want) + b32), 2.0 ** -25)
                err = np.abs(got.astype(np.float64) - want)
                worst = float((err / bound).max())
                print("%s K=%d frame %d level %d %s: worst |err| / bound %.3f, max |err| %.3e" % (name, K, f, l, what, worst, float(err.max())))
                assert np.isfinite(got.astype(np.float32)).all()
                assert (err <= bound).all(), "%s K=%d frame %d level %d %s: %d of %d elements beyond the bound (worst %.3f x)" % (
                    name, K, f, l, what, int((err > bound).sum()), err.size, worst)
                total += err.size
    print("%s K=%d: %d elements within the bound" % (name, K, total))
    plan.close()


@pytest.mark.parametrize("name", ["config1", "reference_crop", "odd"])
def test_null_outputs_and_the_two_parts(rt, name):
    import torch
    from pysilent_amd import _lib
    hw, levels = _levels(name)
    plan = rt.PyramidPlan(hw[0], hw[1], 1, levels, 0)
    frames = np.stack([noise_frame(21, hw[0], hw[1], 1), structured_frame(22, hw[0], hw[1], 1)])
    K = 4
    pyr, cs, end = _pass16(plan, frames, K)
    p1, c1, e1 = _pass16(plan, frames, K, want_end=False)
    assert e1 is None and np.array_equal(_half_bits(c1), _half_bits(cs)) and np.array_equal(p1, pyr)
    p2, c2, e2 = _pass16(plan, frames, K, want_cs=False)
    assert c2 is None and np.array_equal(_half_bits(e2), _half_bits(end)) and np.array_equal(p2, pyr)
    # device form: parts = 1 then parts = 2 on poisoned buffers == parts = 3
    cs_k, end_k = _consts(K)
    n, px = len(frames), plan.frame_px
    fr = torch.from_numpy(frames).cuda(0)
    s = torch.cuda.current_stream().cuda_stream

    def run(parts_seq):
        p = torch.full((n * px,), -7.0, dtype=torch.float32, device="cuda:0")
        c = torch.full((n * px,), 3.0, dtype=torch.float16, device="cuda:0")
        e = torch.full((n * px * K,), 3.0, dtype=torch.float16, device="cuda:0")
        for parts in parts_seq:
            plan.ctx.check(_lib.load().silent_gray_pass_h_dev(
                plan.ctx.handle, plan.handle, fr.data_ptr(), n, cs_k.ctypes.data, end_k.ctypes.data, K, 255.0, p.data_ptr(),
                _lib.half_ptr(c.data_ptr()), _lib.half_ptr(e.data_ptr()), parts, s))
        torch.cuda.synchronize()
        return p.cpu().numpy(), c.cpu().numpy(), e.cpu().numpy()

    whole, halves = run([3]), run([1, 2])
    assert np.array_equal(whole[0], pyr)
    for a, b, ref in zip(whole[1:], halves[1:], (cs, end)):
        assert np.array_equal(_half_bits(a), _half_bits(ref)), "the device form differs from the host form"
        assert np.array_equal(_half_bits(a), _half_bits(b)), "parts 1 + 2 differ from parts = 3"
    plan.close()


def _gray_pipe(hw, K, batch, **kw):
    from pysilent_amd.pipeline import LineEndPipeline
    kw.setdefault("placement", None)
    return LineEndPipeline(hw, mode="gray", n_orient=K, batch=batch, device=0, **kw)


def _maps(out):
    return {k: out[k].data.clone() for k in ("pyramid", "cs", "end")}


def _same_maps(a, b):
    import torch
    ok = True
    for k in a:
        if a[k].dtype != b[k].dtype:
            return False
        v = torch.int32 if a[k].dtype == torch.float32 else torch.int16
        ok = ok and torch.equal(a[k].view(v), b[k].view(v))
    return ok


@pytest.mark.parametrize("hw,K", [((540, 960), 4), ((271, 481), 8)])
def test_pipeline_float16_step_step_host_overlap_and_placement_agree(rt, hw, K):
    import torch
    batch = 2
    u8 = np.stack([np.random.default_rng(40 + i).integers(0, 256, (hw[0], hw[1], 1)).astype(np.uint8) for i in range(batch)])
    f32 = torch.from_numpy(u8.astype(np.float32)).cuda(0)
    ref = _gray_pipe(hw, K, batch)
    ref.step(f32)
    r = ref.outputs()
    base = _gray_pipe(hw, K, batch, storage="float16")
    assert base.storage == "float16" and "float16" in base.launch_summary()
    assert base.cs.dtype == torch.float16 and base.end.dtype == torch.float16 and base.pyr.dtype == torch.float32
    assert base.end.numel() * base.end.element_size() * 2 == ref.end.numel() * ref.end.element_size()
    assert base.algorithmic_bytes_per_frame() == ref.algorithmic_bytes_per_frame() - 2 * base.frame_px * (1 + K)
    assert base.filter_bytes_per_frame() == ref.filter_bytes_per_frame() - 2 * base.frame_px * (1 + K)
    base.step(f32)
    o = base.outputs()
    assert o["cs"].dtype == np.float16 and o["end"].dtype == np.float16 and o["pyramid"].dtype == np.float32
    assert o["end"].level(1).dtype == torch.float16 and o["end"].level(1).shape[-1] == K and o["pyramid"].level(1).dtype == torch.float32
    want = _maps(o)
    # the pipeline's float16 maps are the casts of the float32 pipeline's (torch's cast rounds to nearest even too)
    assert torch.equal(want["pyramid"].view(torch.int32), r["pyramid"].data.view(torch.int32))
    for k in ("cs", "end"):
        assert torch.equal(want[k].view(torch.int16), r[k].data.to(torch.float16).view(torch.int16)), k
    ov = _gray_pipe(hw, K, batch, storage="float16", overlap="force")
    ov.step(f32)
    ov.step(f32)
    assert _same_maps(_maps(ov.outputs()), want), "overlap='force' differs from step"
    host = _gray_pipe(hw, K, batch, storage="float16")
    host.step_host(u8)
    assert _same_maps(_maps(host.outputs()), want), "step_host (uint8) differs from step"
    tuned = _gray_pipe(hw, K, batch, storage="float16", placement="auto")
    tuned.step(f32)
    assert tuned.placement_tuning is not None and tuned.cs.dtype == torch.float16
    assert _same_maps(_maps(tuned.outputs()), want), "the placement tuner changed the float16 maps"
    with pytest.raises(ValueError, match="float16"):
        base.run_filters()
    for p in (ref, base, ov, host, tuned):
        p.close()


def test_storage_float32_is_the_default_path(rt):
    import torch
    hw, K, batch = (540, 960), 4, 2
    f32 = torch.from_numpy(np.stack([noise_frame(50 + i, hw[0], hw[1], 1) for i in range(batch)])).cuda(0)
    a = _gray_pipe(hw, K, batch)
    a.step(f32)
    b = _gray_pipe(hw, K, batch, storage="float32")
    b.step(f32)
    assert a.storage == "float32" and b.storage == "float32" and a.launch_summary() == b.launch_summary()
    assert b.cs.dtype == torch.float32 and b.end.dtype == torch.float32
    assert a.algorithmic_bytes_per_frame() == b.algorithmic_bytes_per_frame()
    assert _same_maps(_maps(a.outputs()), _maps(b.outputs())), "storage='float32' differs from the default"
    for p in (a, b):
        p.close()
