"""float16 storage of the RGB chain's orient and line_end maps (silent_rgb_line_end_h / silent_rgb_keypoints_h, rgb_storage="float16").

The reference of every map test is the float32 entry point with the same arguments: the float16 call must store exactly its elements
rounded once to binary16 (numpy's astype(float16): nearest even, overflow to inf, subnormals kept), NaNs at the same positions, and a
bit-identical float32 value map.  One packed pyramid whose rows start off the dword grid (odd widths, an odd frame_px), whose widths
cross the 112-column wave edge by +-1 and whose levels end in a last odd column or not; at the model's tile height and at 4- and
32-row tiles; on the reference's weights (the symmetric form) and one set each for the dense, basic and two-group forms."""
import ctypes as C

import numpy as np
import pytest

import chain_weights as cw
import err_bound as eb
import silent_oracle as so
from pysilent_amd import _lib
from pysilent_amd._lib import TUNE_RGB

pytestmark = pytest.mark.gpu

EXTENTS = [(1, 1), (2, 3), (5, 113), (9, 225), (33, 112), (17, 224), (40, 130)]
N_FRAMES = 2
FRAME_PX = sum(h * w for h, w in EXTENTS)
assert FRAME_PX == 15301 and FRAME_PX % 2 == 1          # frame 1 and most rows start on a 2-byte boundary only
WEIGHTS = ["reference", "dense", "basic_blur", "two_group"]
VARIANT = {"reference": 3, "dense": 0, "basic_blur": 1, "two_group": 2}
TILES = {"model": None, "4 rows": 2 << 8, "32 rows": 16 << 8}      # SILENT_TUNE_RGB bits 8 - 15: tile height / 2


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _weights(name):
    if name == "reference":
        ref = cw.reference()
        return {k: ref[k] for k in cw.RGB_NAMES}
    return cw.rgb_weights(name)


_NOISE = {}


def _noise():
    if not _NOISE:
        rng = np.random.default_rng(16)
        _NOISE["x"] = (rng.random(N_FRAMES * FRAME_PX * 3) * 255.0).astype(np.float32)
    return _NOISE["x"]


def _input(kind):
    """(flat float32 pyramid, clip_hi)"""
    x = _noise().copy()
    if kind == "noise":
        return x, 255.0
    if kind == "nonfinite":
        rng = np.random.default_rng(17)
        at = rng.choice(x.size, 40, replace=False)
        x[at[:20]] = np.nan
        x[at[20:30]] = np.inf
        x[at[30:]] = -np.inf
        return x, 255.0
    if kind == "tiny":
        return x * np.float32(2.0 ** -20), 255.0
    if kind == "huge":
        return x * np.float32(1e4), 1e6
    raise KeyError(kind)


INPUTS = ["noise", "nonfinite", "tiny", "huge"]


def _packed(rt, flat):
    import torch
    return rt.PackedPyramid(torch.from_numpy(flat).cuda(), EXTENTS, 3, N_FRAMES)


def _host(p):
    return p.data.cpu().numpy()


def _assert_rounded(h, f, what):
    """h: float16 array, f: the float32 array it must be the rounding of."""
    assert h.dtype == np.float16 and f.dtype == np.float32 and h.shape == f.shape, what
    with np.errstate(over="ignore"):
        want = f.astype(np.float16)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(h), nan), "%s: NaN positions differ" % what
    a, b = h.view(np.uint16)[~nan], want.view(np.uint16)[~nan]
    bad = a != b
    assert not bad.any(), "%s: %d of %d elements are not the rounded float32 element (first at %d: %#06x, want %#06x)" % (
        what, bad.sum(), bad.size, int(np.argmax(bad)), int(a[np.argmax(bad)]), int(b[np.argmax(bad)]))


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), "%s: NaN positions differ" % what
    np.testing.assert_array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32), err_msg=what)


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("name", WEIGHTS)
def test_maps_are_the_float32_maps_rounded_once(rt, name, tile):
    ks = _weights(name)
    n_used, variant = C.c_int(0), C.c_int(-1)
    stream = (C.c_float * 384)()
    fp = C.POINTER(C.c_float)
    arrs = [np.ascontiguousarray(ks[k], np.float32) for k in cw.RGB_NAMES]
    prm = _lib.RgbChainParams(*[a.ctypes.data_as(fp) for a in arrs], 1.0, 0.1, _lib.FLAT_IEEE, 255.0, 2)
    assert _lib.load().silent_rgb_chain_stream(C.byref(prm), 0, stream, C.byref(n_used), C.byref(variant)) == 0
    assert variant.value == VARIANT[name], "the weights must take the %s form" % name

    def run():
        for kind in INPUTS:
            flat, clip = _input(kind)
            x = _packed(rt, flat)
            f = rt.rgb_line_end(x, ks, clip_hi=clip)
            h = rt.rgb_line_end(x, ks, clip_hi=clip, storage="float16")
            what = "%s %s %s" % (name, tile, kind)
            fo, fl, fv = _host(f["orient"]), _host(f["line_end"]), _host(f["value"])
            ho, hl = _host(h["orient"]), _host(h["line_end"])
            _assert_rounded(ho, fo, "orient " + what)
            _assert_rounded(hl, fl, "line_end " + what)
            _same_bits(_host(h["value"]), fv, "value " + what)
            assert h["line_end"].level(3).shape == (N_FRAMES, 9, 225, 3)
            if kind == "nonfinite":
                assert np.isnan(hl).any() and np.isnan(ho).any()
            if kind == "tiny":      # binary16 subnormals are kept: stored values below 2^-14 that are not zero
                for m in (ho, hl):
                    mag = np.abs(m.astype(np.float32))
                    assert ((mag < 2.0 ** -14) & (mag > 0)).any(), what
            if kind == "huge":      # line_end passes 65504: +inf exactly where the float32 value rounds so
                assert (fl[np.isfinite(fl)] > 65504.0).any() and np.isposinf(hl).any(), what
                assert np.array_equal(np.isposinf(hl), np.nan_to_num(fl, nan=0.0) >= 65520.0), what

    if TILES[tile] is None:
        run()
    else:
        with rt.tuning(TUNE_RGB, TILES[tile]):
            run()


@pytest.mark.parametrize("absent", ["orient", "line_end", "value"])
def test_each_output_may_be_null(rt, absent):
    ks = _weights("reference")
    flat, clip = _input("noise")
    x = _packed(rt, flat)
    want = tuple(n for n in ("orient", "line_end", "value") if n != absent)
    f = rt.rgb_line_end(x, ks, want=want)
    h = rt.rgb_line_end(x, ks, want=want, storage="float16")
    assert sorted(h) == sorted(want)
    for n in want:
        if n == "value":
            _same_bits(_host(h[n]), _host(f[n]), "value without " + absent)
        else:
            _assert_rounded(_host(h[n]), _host(f[n]), "%s without %s" % (n, absent))


def test_against_the_cpu_oracle(rt):
    """Sanity bound: |float(h) - oracle| <= the float32 bound of that map (tests/err_bound.py; 1e-5 range-relative where the bound is
    not finite) + the binary16 rounding bound (2^-11 relative, 2^-25 absolute below 2^-14)."""
    ks = _weights("reference")
    flat, clip = _input("noise")
    h = rt.rgb_line_end(_packed(rt, flat), ks, storage="float16")
    per_frame = flat.reshape(N_FRAMES, FRAME_PX * 3)
    off = 0
    for l, (eh, ew) in enumerate(EXTENTS):
        lev = np.ascontiguousarray(per_frame[:, off * 3:(off + eh * ew) * 3].reshape(N_FRAMES, eh, ew, 3))
        off += eh * ew
        want = so.rgb_line_end_chain(lev, ks, "ieee")
        bound = eb.rgb_chain(lev, ks, want, "ieee")
        for got, w, b in ((h["orient"].level(l), want["orient"], bound["orient"]), (h["line_end"].level(l), want["padded"], bound["padded"])):
            g = got.cpu().numpy().astype(np.float64)
            w = np.asarray(w, np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(w))
            fin = ~np.isnan(w)
            scale = float(np.abs(w[fin]).max()) if fin.any() else 1.0
            b32 = np.where(np.asarray(b, np.float64) < 1e29, b, 1e-5 * (np.abs(w) + scale))
            b16 = np.maximum(2.0 ** -11 * (np.abs(w) + b32), 2.0 ** -25)
            err = np.abs(g - w)[fin]
            assert (err <= (b32 + b16)[fin] + 1e-38).all(), "level %d: worst excess %.3e" % (l, float((err - (b32 + b16)[fin]).max()))


# ----------------------------------------------------------------------------- keypoints

REGIONS = [(max(h // 2, 1), max(w // 2, 1)) for h, w in EXTENTS]


def _kp_calls(rt, flat, ks, top_percent, peak_map, clip=255.0, regions=None):
    """(h: silent_rgb_keypoints_h_dev, pair: silent_rgb_line_end_h_dev + silent_select_keypoints_dev on the widened line_end,
    f32: silent_rgb_keypoints_dev) -> dicts of host arrays; stats: the sparse tail's of the _h call.  regions: one (rH, rW) per
    level of EXTENTS (default: REGIONS, half the level)."""
    import torch
    lib = _lib.load()
    ctx = rt.get_context(0)
    dev = torch.device("cuda", 0)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    x = torch.from_numpy(flat).to(dev)
    lv = (_lib.Extent * len(EXTENTS))(*[_lib.Extent(h, w) for h, w in EXTENTS])
    rg = (_lib.Extent * len(EXTENTS))(*[_lib.Extent(int(h), int(w)) for h, w in (REGIONS if regions is None else regions)])
    assert len(rg) == len(EXTENTS)
    fp = C.POINTER(C.c_float)
    arrs = [np.ascontiguousarray(ks[k], np.float32) for k in cw.RGB_NAMES]
    prm = _lib.RgbChainParams(*[a.ctypes.data_as(fp) for a in arrs], 1.0, 0.1, _lib.FLAT_IEEE, float(clip), 2)
    n, cap = N_FRAMES * FRAME_PX, FRAME_PX
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    hp = lambda t: _lib.half_ptr(t.data_ptr())

    def bufs(dt):
        return dict(orient=torch.full((n * 3,), 7, dtype=dt, device=dev), line_end=torch.full((n * 3,), 7, dtype=dt, device=dev),
                    value=torch.full((n,), 7, dtype=torch.float32, device=dev),
                    peak=torch.full((n,), 7, dtype=torch.float32, device=dev) if peak_map else None,
                    idx=torch.zeros((N_FRAMES, cap, 4), dtype=torch.int64, device=dev), counts=torch.zeros(N_FRAMES, dtype=torch.int64, device=dev))
    geom = (lv, len(EXTENTS), N_FRAMES)
    h = bufs(torch.float16)
    ctx.check(lib.silent_rgb_keypoints_h_dev(ctx.handle, p(x), *geom, C.byref(prm), C.c_double(top_percent), rg, hp(h["orient"]), hp(h["line_end"]),
                                             p(h["value"]), p(h["peak"]), p(h["idx"]), cap, p(h["counts"]), s))
    st = (C.c_int64 * 5)()
    ctx.check(lib.silent_sparse_tail_stats(ctx.handle, st))
    pair = bufs(torch.float16)
    ctx.check(lib.silent_rgb_line_end_h_dev(ctx.handle, p(x), *geom, C.byref(prm), hp(pair["orient"]), hp(pair["line_end"]), p(pair["value"]), s))
    wide = pair["line_end"].to(torch.float32)
    ctx.check(lib.silent_select_keypoints_dev(ctx.handle, p(wide), p(pair["value"]), *geom, 3, C.c_double(top_percent), rg, p(pair["peak"]),
                                              p(pair["idx"]), cap, p(pair["counts"]), s))
    f = bufs(torch.float32)
    ctx.check(lib.silent_rgb_keypoints_dev(ctx.handle, p(x), *geom, C.byref(prm), C.c_double(top_percent), rg, p(f["orient"]), p(f["line_end"]),
                                           p(f["value"]), p(f["peak"]), p(f["idx"]), cap, p(f["counts"]), s))
    torch.cuda.synchronize()
    host = lambda d: {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}
    return host(h), host(pair), host(f), [int(v) for v in st]


def _rows(d, f):
    return d["idx"][f, :int(d["counts"][f])]


def _assert_same_keypoints(h, pair, what):
    np.testing.assert_array_equal(h["counts"], pair["counts"], err_msg=what)
    assert (h["counts"] <= FRAME_PX).all()
    for f in range(N_FRAMES):
        np.testing.assert_array_equal(_rows(h, f), _rows(pair, f), err_msg=what)
    for m in ("orient", "line_end"):
        np.testing.assert_array_equal(h[m].view(np.uint16), pair[m].view(np.uint16), err_msg=what + " " + m)
    _same_bits(h["value"], pair["value"], what + " value")
    if h["peak"] is not None:
        _same_bits(h["peak"], pair["peak"], what + " peak_value")


def _differing(h, f):
    n = 0
    for fr in range(N_FRAMES):
        a, b = {tuple(r) for r in _rows(h, fr)}, {tuple(r) for r in _rows(f, fr)}
        n += len(a ^ b)
    return n


@pytest.mark.parametrize("peak_map", [False, True])
@pytest.mark.parametrize("top_percent", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("name", ["reference", "two_group", "dense"])
def test_keypoints_equal_the_pair_of_calls(rt, name, top_percent, peak_map):
    """silent_rgb_keypoints_h_dev = silent_rgb_line_end_h_dev + silent_select_keypoints_dev(color = widened line_end, value = the
    float32 value map): indices, counts and peak values bit for bit.  Without a peak-value map the reference's and the two-group
    weights take the sparse route (the dense weights have no extrema instantiation: reduction pass + dense kernels)."""
    ks = _weights(name)
    flat, _ = _input("noise")
    h, pair, f, st = _kp_calls(rt, flat, ks, top_percent, peak_map)
    _assert_same_keypoints(h, pair, "%s p=%g map=%s" % (name, top_percent, peak_map))
    assert bool(st[0]) == (name != "dense"), st
    assert int(h["counts"].sum()) > 0
    print("keypoints that differ from the float32 call's (%s, p = %g): %d of %d" % (name, top_percent, _differing(h, f), int(f["counts"].sum())))


@pytest.mark.parametrize("peak_map", [False, True])
def test_keypoints_on_the_dense_route(rt, peak_map):
    """A level with a NaN and an all-zero level: the sparse tail hands those (frame, level)s to the dense kernels / the synthesised
    map; same contract."""
    ks = _weights("reference")
    flat, _ = _input("noise")
    flat = flat.copy()
    per = flat.reshape(N_FRAMES, FRAME_PX, 3)
    off = [sum(h * w for h, w in EXTENTS[:l]) for l in range(len(EXTENTS) + 1)]
    per[0, off[4] + 7 * 112 + 50, 1] = np.nan              # frame 0, level (33, 112)
    per[1, off[5]:off[6]] = 0.0                            # frame 1, level (17, 224): all zero
    per[0, off[3]:off[4]] = 0.0                            # frame 0, level (9, 225): all zero next to the NaN level
    h, pair, f, st = _kp_calls(rt, flat, ks, 0.1, peak_map)
    _assert_same_keypoints(h, pair, "dense route map=%s" % peak_map)
    assert st[0] == 1 and st[2] + st[4] >= 2, st           # dense pairs + synthesised zero maps
    assert np.isnan(h["value"]).any()


@pytest.mark.parametrize("peak_map", [False, True])
@pytest.mark.parametrize("name", ["reference", "two_group"])
def test_keypoints_with_a_clip_bound_beyond_binary16(rt, name, peak_map):
    """clip_hi = 1e6 on noise x 1e4: line_end is stored as +inf where it passes 65504, and +inf times the 0 of a pixel below the
    threshold is a NaN peak value at a pixel whose VALUE is no NaN.  The sparse tail places NaNs by the value map's flags only, so the
    call must keep the dense kernels there -- and equal the pair of calls, as everywhere."""
    ks = _weights(name)
    flat, clip = _input("huge")
    h, pair, f, st = _kp_calls(rt, flat, ks, 0.1, peak_map, clip=clip)
    assert np.isposinf(h["line_end"]).any() and not np.isnan(h["value"]).any()
    assert st[0] == 0, st                                   # not the sparse route
    _assert_same_keypoints(h, pair, "%s clip 1e6 map=%s" % (name, peak_map))
    if peak_map:                                            # the case the branch is for: NaN peak values without a NaN value
        assert np.isnan(pair["peak"]).any()


# ----------------------------------------------------------------------------- pipeline

HW = (96, 150)


def _frames(seed=5, batch=2):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (batch,) + HW + (3,)).astype(np.float32)


def _pipes(**kw):
    from pysilent_amd.pipeline import LineEndPipeline
    common = dict(mode="rgb", n_levels=3, batch=2, max_keypoints_per_frame=1 << 15, placement=None)     # ("plain" below: placement="auto")
    common.update(kw)
    return LineEndPipeline(HW, **common), LineEndPipeline(HW, rgb_storage="float16", **common)


def _assert_pipeline_maps(a, b, what):
    """a: float32 pipeline's outputs, b: the float16 one's."""
    for m in ("orient", "line_end"):
        assert b[m].dtype == np.float16 and b[m].data.element_size() == 2 and b[m].extents == a[m].extents and b[m].channels == 3
        assert b[m].level(1).shape == a[m].level(1).shape
        _assert_rounded(b[m].data.cpu().numpy(), a[m].data.cpu().numpy(), "%s %s" % (what, m))
    _same_bits(b["value"].data.cpu().numpy(), a["value"].data.cpu().numpy(), what + " value")
    _same_bits(b["pyramid"].data.cpu().numpy(), a["pyramid"].data.cpu().numpy(), what + " pyramid")


def _assert_same_rows(a, b, what):
    np.testing.assert_array_equal(a["keypoint_counts"], b["keypoint_counts"], err_msg=what)
    for f in range(len(a["keypoints"])):
        np.testing.assert_array_equal(a["keypoints"][f], b["keypoints"][f], err_msg=what)


def test_pipeline_without_selection_and_with_attention(rt):
    """selection=False: keypoints, value, and the attention outputs and state after three steps equal the float32 pipeline's bit for bit."""
    import torch
    f32, f16 = _pipes(attention=True)
    for step in range(3):
        t = torch.from_numpy(_frames(5 + step)).cuda()
        f32.step(t)
        f16.step(t)
    torch.cuda.synchronize()
    a, b = f32.outputs(), f16.outputs()
    _assert_pipeline_maps(a, b, "attention")
    _assert_same_rows(a, b, "attention")
    assert int(a["keypoint_counts"].sum()) > 0
    for m in ("centroids", "centroids2", "fired", "update"):
        _same_bits(b[m].data.cpu().numpy(), a[m].data.cpu().numpy(), m)
    _same_bits(f16.energy.cpu().numpy(), f32.energy.cpu().numpy(), "energy")


def _entry_point_rows(pipe):
    """silent_rgb_keypoints_h_dev on the pipeline's own pyramid, into fresh buffers."""
    import torch
    lib = _lib.load()
    n = pipe.batch * pipe.frame_px
    dev = pipe.tdev
    o, l = (torch.empty(n * 3, dtype=torch.float16, device=dev) for _ in range(2))
    idx = torch.zeros((pipe.batch, pipe.kp_cap, 4), dtype=torch.int64, device=dev)
    counts = torch.zeros(pipe.batch, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    pipe.ctx.check(lib.silent_rgb_keypoints_h_dev(
        pipe.ctx.handle, p(pipe.pyr), pipe.levels_c, pipe.n_levels, pipe.batch, C.byref(pipe._params), C.c_double(pipe.top_percent), pipe.regions,
        _lib.half_ptr(o.data_ptr()), _lib.half_ptr(l.data_ptr()), None, None, p(idx), pipe.kp_cap, p(counts),
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    return {"keypoint_counts": c, "keypoints": [idx[f, :int(c[f])].cpu().numpy() for f in range(pipe.batch)]}, o.cpu().numpy(), l.cpu().numpy()


@pytest.mark.parametrize("case", ["plain", "no orient map", "nv12", "overlap"])
def test_pipeline_with_selection_equals_the_entry_point(rt, case):
    import torch
    kw = dict(selection=True)
    frames = torch.from_numpy(_frames()).cuda()
    if case == "no orient map":
        kw.update(orient_map=False, value_map=False, peak_value_map=False)
    if case == "nv12":
        kw.update(rgb_frame_format="nv12")
        rng = np.random.default_rng(9)
        frames = (torch.from_numpy(rng.integers(16, 236, (2,) + HW, dtype=np.uint8)).cuda(),
                  torch.from_numpy(rng.integers(16, 241, (2, HW[0] // 2, HW[1] // 2, 2), dtype=np.uint8)).cuda())
    if case == "overlap":
        kw.update(overlap="force")
    if case == "plain":
        kw.update(placement="auto")         # the tuner redraws the maps: allocated by element size
    f32, f16 = _pipes(**kw)
    for _ in range(2):                      # (overlap: both pyramid buffers have been used)
        f32.step(frames)
        f16.step(frames)
    f32.wait()
    f16.wait()
    torch.cuda.synchronize()
    a, b = f32.outputs(), f16.outputs()
    want, o, l = _entry_point_rows(f16)
    _assert_same_rows(want, b, case)
    np.testing.assert_array_equal(b["line_end"].data.cpu().numpy().view(np.uint16), l.view(np.uint16))
    _assert_rounded(b["line_end"].data.cpu().numpy(), a["line_end"].data.cpu().numpy(), case + " line_end")
    if case == "no orient map":
        assert "orient" not in b and "value" not in b
    else:
        _assert_pipeline_maps(a, b, case)
        np.testing.assert_array_equal(b["orient"].data.cpu().numpy().view(np.uint16), o.view(np.uint16))
    assert int(b["keypoint_counts"].sum()) > 0


def test_per_op_path_raises(rt):
    _, f16 = _pipes()
    with pytest.raises(ValueError, match="rgb_storage='float16' has no per-op filter pass"):
        f16.run_filters()
    with pytest.raises(ValueError, match="rgb_storage='float16' has no per-op keypoint pass"):
        f16.run_keypoints()
    # the fused float32 step would write 12 bytes per pixel into the 6-byte maps: refused before any call
    for pipe in (f16, _pipes(selection=True)[1]):
        with pytest.raises(ValueError, match="rgb_storage='float16' has no float32 fused step"):
            pipe.run_filters_keypoints()
