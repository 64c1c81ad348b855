"""The case table of tests/test_gpu_write_coverage.py (plain module: tests/test_write_coverage.py checks its staging bounds on the
CPU).  A case is (id, calls(rt, *inputs) -> list of CALLS, inputs): a call is a function without arguments that makes ONE library
call on the inputs -- NumPy arrays (host forms) or the same values on the GPU (device forms) -- and returns its results as a tuple.
The tests treat every call on its own: the staging arena is poisoned before each, and each is run after a call of its own geometry
on other values.  Shapes are the ones the suite already trusts, the smallest at which tails and tiles can go wrong; nothing here is
workload-sized.

Results compared only in part (write_coverage.Rows), everything else element for element:
  * keypoint index rows past counts[f] -- include/silent_hip.h:344-346 ("counts[f] = number of rows frame f produced.  If any
    count exceeds cap_per_frame only the first cap_per_frame rows of that frame are written"): every case whose id starts with
    max_value_indices_region, select_keypoints, rgb_keypoints, gray_keypoints, tiny or overflow.
"""
import ctypes as C
import math

import numpy as np

import chain_weights as cw
import plan_geometry as pg
import write_coverage as wc

E5 = float(math.e) ** .5


class Case(object):
    """``out_bytes``: an upper bound of the bytes of the results of any ONE call of the case; ``default_route``: no kernel-selection
    knob is set (the case also runs with the weakest result alignment); ``workspace``: the entry point keeps intermediates in the
    context workspace (the previous-call test)."""

    def __init__(self, id, calls, make_inputs, out_bytes, default_route=True, workspace=False):
        self.id, self.calls, self._make, self.out_bytes = id, calls, make_inputs, int(out_bytes)
        self.default_route, self.workspace = default_route, workspace
        self._inputs = None

    def inputs(self):
        """Built once, read-only."""
        if self._inputs is None:
            self._inputs = tuple(self._make())
            for a in self._inputs:
                raw(a).setflags(write=False)
        return self._inputs

    def input_bytes(self):
        return [raw(a).nbytes for a in self.inputs()]

    def staging_bound(self):
        """Arena bytes one host-form call of this case can need: every input of the case, the results of one call, each rounded up,
        plus 1 MiB for what is not an array of the case (weights, region tables)."""
        return wc.staged_bytes(self.input_bytes()) + self.out_bytes + 16 * wc.ARENA_ALIGN + (1 << 20)


CASES = []


def case(id, calls, make_inputs, out_bytes, **kw):
    CASES.append(Case(id, calls, make_inputs, out_bytes, **kw))


def _tuple(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def each(f):
    """calls of a case: the calls ``f(rt, x)`` lists, for every input x."""
    def calls(rt, *xs):
        return [c for x in xs for c in f(rt, x)]
    return calls


def one(g):
    """f of each() for an op that is one call: g(rt, x) -> results."""
    return lambda rt, x: [lambda: _tuple(g(rt, x))]


def knobbed(rt, which, value, call):
    """``call`` with a kernel-selection knob of the context set for its duration."""
    def run():
        with rt.tuning(which, value):
            return call()
    return run


# ----------------------------------------------------------------------------- inputs

class Packed(object):
    """A host PackedPyramid before there is a runtime: data + geometry (rt.PackedPyramid is built in on_host / on_device)."""

    def __init__(self, levels):
        self.levels = levels
        n, c = levels[0].shape[0], levels[0].shape[-1]
        self.extents, self.channels, self.n_frames = [l.shape[1:3] for l in levels], c, n
        self.data = np.concatenate([np.concatenate([np.ascontiguousarray(l[f], np.float32).reshape(-1) for l in levels]) for f in range(n)])


def raw(x):
    """The ndarray behind an input."""
    return x.data if isinstance(x, Packed) else x


def on_host(rt, x):
    if isinstance(x, Packed):
        return rt.PackedPyramid(np.array(x.data), x.extents, x.channels, x.n_frames)
    return np.array(x)


def on_device(rt, x):
    import torch
    if isinstance(x, Packed):
        return rt.PackedPyramid(torch.from_numpy(np.array(x.data)).cuda(0), x.extents, x.channels, x.n_frames)
    return torch.from_numpy(np.array(x)).cuda(0)


def other_values(x, kind):
    """An input of the same geometry and dtype with other values: kind 1 all zero, kind 2 noise of another seed scaled by 0.25."""
    data = raw(x)
    if kind == 1:
        new = np.zeros_like(data)
    else:
        noise = np.random.default_rng(990 + data.size % 7).integers(0, 256, data.shape)
        new = (noise // 4).astype(np.uint8) if data.dtype == np.uint8 else (noise.astype(np.float32) * np.float32(0.25))
    if isinstance(x, Packed):
        p = Packed.__new__(Packed)
        p.levels, p.extents, p.channels, p.n_frames, p.data = None, x.extents, x.channels, x.n_frames, new
        return p
    return new


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.float32)


POINT_SHAPES = [(1, 1, 1), (3, 19, 5), (2, 37, 53)]
RAGGED = [(12, 20), (7, 9), (5, 3)]            # level starts on odd offsets
PX = max(max(n * h * w for n, h, w in POINT_SHAPES), 2 * sum(h * w for h, w in RAGGED))         # pixels of the largest pointwise input


def point_inputs(c, seed, sparse=False, scale=None):
    """The pointwise shapes and the ragged packed pyramid, ``c`` channels."""
    def make():
        xs = [noise(s + (c,), seed + i) for i, s in enumerate(POINT_SHAPES)] + [Packed([noise((2, h, w, c), seed + 9 + h) for h, w in RAGGED])]
        for x in xs:
            d = raw(x)
            if sparse:           # (centroids: empty cells)
                d[np.random.default_rng(seed).random(d.shape) > 0.4] = 0.0
            if scale is not None:
                d *= np.float32(scale)
        return xs
    return make


# ----------------------------------------------------------------------------- pointwise / selection

case("pad_inwards", each(one(lambda rt, x: rt.pad_inwards(x, 2, 1, 3, 2))), point_inputs(3, 10), PX * 12)
case("value_from_color", each(one(lambda rt, x: rt.value_from_color(x))), point_inputs(3, 20), PX * 4)
case("bw_from_color", each(one(lambda rt, x: rt.bw_from_color(x))), point_inputs(3, 30), PX * 4)
case("nms3x3-product", each(one(lambda rt, x: rt.nms3x3(x, "product"))), point_inputs(3, 40), PX * 12)
case("nms3x3-fired", each(one(lambda rt, x: rt.nms3x3(x, "fired"))), point_inputs(1, 50), PX * 4)
case("top_value_points", each(one(lambda rt, x: rt.top_value_points(x, 0.1))), point_inputs(3, 60), PX * 12)
case("affine_clip", each(one(lambda rt, x: rt.affine_clip(x, 255.0 / 4.0, 0.0, 1.0, 256.0, -1.0))), point_inputs(3, 70), PX * 12)
for _c in (1, 3):
    case("select_peaks-c%d" % _c, each(one(lambda rt, x: tuple(rt.select_peaks(x, 0.1)[k] for k in ("top", "peaks", "peak_value")))),
         point_inputs(_c, 80 + _c), PX * 4 * (2 * _c + 1), workspace=True)


def _resize(rt, x):
    if isinstance(x, rt.PackedPyramid):
        return rt.resize_nearest(x, [(2 * h + 1, max(w - 2, 1)) for h, w in x.extents])
    h, w = x.shape[1:3]
    return rt.resize_nearest(x, (2 * h + 1, max(w - 2, 1)))


case("resize_nearest", each(one(_resize)), point_inputs(3, 90), PX * 3 * 12)
case("centroids", each(one(lambda rt, x: rt.centroids(x, 3, 3))), point_inputs(1, 100, sparse=True), PX * 8, workspace=True)


def _boosting(visualize):
    def g(rt, x):
        """The state lies between guards of its own: it is an output too (updated in place)."""
        packed = isinstance(x, rt.PackedPyramid)
        src = x.data if packed else x
        state = wc.result_like(src, tuple(src.shape))
        if hasattr(state, "fill_"):
            state.fill_(8.0)
        else:
            state[...] = 8
        fired, energy = rt.boosting_step(x, rt.PackedPyramid(state, x.extents, 1, x.n_frames) if packed else state, visualize=visualize)
        return fired, energy, state
    return g


case("boosting_step", each(one(_boosting(False))), point_inputs(1, 110, scale=1.0 / 255.0), PX * 4 * 3)
case("boosting_step-visualize", each(one(_boosting(True))), point_inputs(1, 120, scale=1.0 / 255.0), PX * 4 * 7)


def _cast_interleave(rt, x):
    """uint8 pixels widened whole, and plane 1 cut out of the interleaved image: silent_cast_interleave[_dev] writes exactly
    (n_pixels - 1) * out_stride + out_offset + count floats."""
    from pysilent_amd import _lib
    n_px = int(np.prod(x.shape)) // 3
    flat = x.reshape(-1)

    def cast(in_off, count, out_stride):
        def run():
            out = wc.result_like(x, (n_px * out_stride,))
            if hasattr(x, "data_ptr"):
                rt.cast_interleave(flat, out, 3, in_off, count, out_stride, 0, n_px)
            else:
                ctx, lib = rt.get_context(), _lib.load()
                ctx.check(lib.silent_cast_interleave(ctx.handle, C.c_void_p(flat.ctypes.data), _lib.DT_U8, n_px, 3, in_off, count,
                                                     C.c_void_p(out.ctypes.data), out_stride, 0))
            return (out,)
        return run
    return [cast(0, 3, 3), cast(1, 1, 1)]


case("cast_interleave", each(_cast_interleave), lambda: [noise(s + (3,), 130 + i).astype(np.uint8) for i, s in enumerate(POINT_SHAPES)], PX * 12)


# ----------------------------------------------------------------------------- conv2d_same / regulate

CONV_KSHAPES = [(3, 3, 1, 1), (3, 3, 1, 3), (3, 3, 1, 4), (3, 3, 1, 8), (3, 3, 3, 1), (3, 3, 3, 4), (7, 7, 1, 1), (5, 5, 3, 2), (2, 2, 3, 3),
                (1, 3, 3, 3), (4, 6, 2, 5)]          # test_conv2d_shapes_including_generic_path
CONV_X = [(2, 23, 71), (1, 17, 130)]                 # 64-pixel tile rows plus a tail of 7 and of 2
CONV_PX = max(n * h * w for n, h, w in CONV_X)


def _conv_inputs(c):
    return lambda: [(np.random.default_rng(11 + i).standard_normal(s + (c,)) * 40).astype(np.float32) for i, s in enumerate(CONV_X)]


for _ks in CONV_KSHAPES:
    _k = np.random.default_rng(11).standard_normal(_ks)
    case("conv2d_same-%dx%dx%dx%d" % _ks,
         each(lambda rt, x, k=_k: [lambda: (rt.conv2d_same(x, k),), lambda: (rt.conv2d_same(x, k, relu=True, clip_hi=30.0),)]),
         _conv_inputs(_ks[2]), CONV_PX * _ks[3] * 4)

for _ks in [(3, 3, 1, 1), (7, 7, 1, 1), (2, 2, 3, 3), (1, 3, 3, 3), (7, 7, 3, 3)]:
    _k = np.abs(np.random.default_rng(12).standard_normal(_ks)) * 1e-3
    case("regulate-%dx%dx%dx%d" % _ks,
         each(lambda rt, x, k=_k: [lambda p=p: (rt.regulate(abs(x), k, 1.0, 0.1, flat_policy=p),) for p in ("ieee", "zero")]),
         _conv_inputs(_ks[2]), CONV_PX * _ks[3] * 4)


# ----------------------------------------------------------------------------- pyramid plans

_PLANS = {}


def plan_of(rt, key, hw, channels, levels, **kw):
    """One plan per (case, flavour) for the life of the process."""
    if key not in _PLANS:
        _PLANS[key] = rt.PyramidPlan(hw[0], hw[1], channels, levels, **kw)
    return _PLANS[key]


def _u8_frames(hw, c, seed, n=2):
    return np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], c)).astype(np.uint8)


def _plan_inputs(hw, channels, seed):
    def make():
        u8 = _u8_frames(hw, channels, seed)
        return [u8.astype(np.float32), u8] + ([_u8_frames(hw, 3, seed + 1)] if channels == 1 else [])
    return make


def _plan_default(name, channels):
    def calls(rt, f32, u8, u8x3=None):
        c = pg.CASES[name]
        plan = plan_of(rt, (name, channels), c["frame"], channels, c["levels"])
        out = [lambda: (plan.run(f32),)]
        if channels == 1:
            out += [lambda: (plan.run(u8, frame_dtype="uint8"),), lambda: (plan.run(u8x3, frame_dtype="uint8", frame_channels=3),)]
        return out
    return calls


def _plan_knobs(name, channels):
    def calls(rt, f32, u8, u8x3=None):
        from pysilent_amd._lib import TUNE_PYRAMID
        c = pg.CASES[name]
        plan = plan_of(rt, (name, channels), c["frame"], channels, c["levels"])
        if (name, channels, "per_level") not in _PLANS:
            with rt.tuning(TUNE_PYRAMID, 4):
                plan_of(rt, (name, channels, "per_level"), c["frame"], channels, c["levels"])
        per_level = _PLANS[(name, channels, "per_level")]
        out = [knobbed(rt, TUNE_PYRAMID, knob, lambda: (plan.run(f32),)) for knob in (1, 2, 8)] + [lambda: (per_level.run(f32),)]
        if channels == 1:
            out += [knobbed(rt, TUNE_PYRAMID, 1, lambda: (plan.run(u8, frame_dtype="uint8"),)),
                    knobbed(rt, TUNE_PYRAMID, 1, lambda: (plan.run(u8x3, frame_dtype="uint8", frame_channels=3),))]
        return out
    return calls


def _levels_px(levels):
    return sum(l[6] * l[7] for l in levels)


for _i, _name in enumerate(sorted(pg.CASES)):
    for _c in (1, 3):
        _px = 2 * _levels_px(pg.CASES[_name]["levels"]) * _c * 4
        case("plan-%s-c%d" % (_name, _c), _plan_default(_name, _c), _plan_inputs(pg.CASES[_name]["frame"], _c, 300 + _i), _px)
        case("plan-%s-c%d-knobs" % (_name, _c), _plan_knobs(_name, _c), _plan_inputs(pg.CASES[_name]["frame"], _c, 300 + _i), _px,
             default_route=False)


# ----------------------------------------------------------------------------- the gray pass

GRAY_FAMILIES = ["ratio2_3", "ratio2_6", "sqrt2_4", "one_level", "reference_crop", "ratio2_3_nostream"]     # tests/test_gray_uint8.py
KS = (3, 4, 8)
FRAME_KINDS = ({}, dict(frame_dtype="uint8"), dict(frame_dtype="uint8", frame_channels=3))        # for inputs (f32, u8, u8x3)


def gray_family_levels(family, hw):
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    if family in ("ratio2_3", "ratio2_3_nostream"):
        return classic_levels(hw, 2.0, 3)
    if family == "ratio2_6":
        return classic_levels(hw, 2.0, 6)
    if family == "sqrt2_4":
        return classic_levels(hw, 2.0 ** .5, 4)
    if family == "one_level":
        return classic_levels(hw, 2.0, 1)
    if family == "reference_crop":
        return reference_levels(hw, (48, 32), E5)
    raise KeyError(family)


def _gray_weights(K):
    return cw.gray_cs(cw.SEED), cw.gray_bank(K, cw.SEED)


def gray_knobbed(rt, family, value, call):
    """SILENT_TUNE_GRAY for the call; the *_nostream family adds bit 4 (16) to whatever is asked for."""
    from pysilent_amd._lib import TUNE_GRAY
    return knobbed(rt, TUNE_GRAY, value | (16 if family.endswith("_nostream") else 0), call)


def _gray_default(family, hw, K):
    def calls(rt, *frames):
        levels = gray_family_levels(family, hw)
        plan = plan_of(rt, ("gray", family, hw), hw, 1, levels)
        plan64 = plan_of(rt, ("gray64", family, hw), hw, 1, levels, accumulation="float64")
        cs_k, bank = _gray_weights(K)
        out = [gray_knobbed(rt, family, 0, lambda fr=fr, kw=kw, st=st: plan.gray_pass(fr, cs_k, bank, storage=st, **kw))
               for st in ("float32", "float16") for fr, kw in zip(frames, FRAME_KINDS)]
        return out + [gray_knobbed(rt, family, 0, lambda: plan64.gray_pass(frames[0], cs_k, bank))]
    return calls


def _gray_knobs(family, hw, K):
    def calls(rt, *frames):
        plan = plan_of(rt, ("gray", family, hw), hw, 1, gray_family_levels(family, hw))
        cs_k, bank = _gray_weights(K)
        return [gray_knobbed(rt, family, knob, lambda fr=fr, kw=kw, st=st: plan.gray_pass(fr, cs_k, bank, storage=st, **kw))
                for knob in (1, 16, 32) for (fr, kw), st in zip(zip(frames, FRAME_KINDS), ("float32", "float16", "float16"))]
    return calls


def gray_keypoints(rt, plan, frames, K, selection=True, kind={}, cap=None, overflow=False):
    """silent_gray_keypoints[_u8[x3]][_dev] through the plan's operand, with the value map and (selection = 1) the peak-value map the
    wrapper never asks for."""
    from pysilent_amd import _lib
    cs_k, bank = [np.ascontiguousarray(np.asarray(k, np.float64).astype(np.float32)) for k in _gray_weights(K)]
    op = plan._frames(frames, **kind)
    n, px = op.n_frames, plan.frame_px
    cap = px if cap is None else cap
    (pyr, pp), (cso, cp), (endo, ep), (value, vp) = [op.empty(n * px * ch) for ch in (1, 1, K, 1)]
    peak, kp = op.empty(n * px) if selection else (None, None)
    idx, iptr = op.empty((n, cap, 4), np.int64)
    counts, cptr = op.empty(n, np.int64)
    reg = (_lib.Extent * len(plan.extents))(*[_lib.Extent(max(h // 2, 1), max(w // 2, 1)) for h, w in plan.extents])
    _call(op, overflow, plan._entry("gray_keypoints", kind.get("frame_dtype", "float32"), kind.get("frame_channels", 1)), plan.handle, op.ptr, n,
          C.c_void_p(cs_k.ctypes.data), C.c_void_p(bank.ctypes.data), K, 255.0, pp, cp, ep, 2, int(selection), 0.1, reg, vp, kp, iptr, cap, cptr)
    if overflow:
        _overflowed(counts, cap)
    return pyr, cso, endo, value, peak, wc.Rows(idx, counts)


def _gray_keypoints(family, hw, K):
    def calls(rt, f32, u8, u8x3):
        plan = plan_of(rt, ("gray", family, hw), hw, 1, gray_family_levels(family, hw))
        return [gray_knobbed(rt, family, 0, lambda sel=sel, fr=fr, kw=kw: gray_keypoints(rt, plan, fr, K, sel, kw))
                for sel, fr, kw in ((True, f32, FRAME_KINDS[0]), (False, u8, FRAME_KINDS[1]), (False, f32, FRAME_KINDS[0]), (True, u8x3, FRAME_KINDS[2]))]
    return calls


for _fi, _family in enumerate(GRAY_FAMILIES):
    for _hw in (pg.FA, pg.FB):
        _px = 2 * sum(l[6] * l[7] for l in gray_family_levels(_family, _hw))
        for _K in KS:
            _tag = "%s-%dx%d-K%d" % (_family, _hw[0], _hw[1], _K)
            case("gray_pass-" + _tag, _gray_default(_family, _hw, _K), _plan_inputs(_hw, 1, 500 + _fi), _px * (2 + _K) * 4,
                 default_route=not _family.endswith("_nostream"))
            case("gray_pass-" + _tag + "-knobs", _gray_knobs(_family, _hw, _K), _plan_inputs(_hw, 1, 500 + _fi), _px * (2 + _K) * 4,
                 default_route=False)
            case("gray_keypoints-" + _tag, _gray_keypoints(_family, _hw, _K), _plan_inputs(_hw, 1, 520 + _fi),
                 _px * ((2 + _K) * 4 + 8 + 32) + 4096, default_route=not _family.endswith("_nostream"), workspace=True)


def _gray_line_end(K):
    def g(rt, x):
        cs_k, bank = _gray_weights(K)
        return rt.gray_line_end(x, cs_k, bank)
    return g


for _K in KS:
    case("gray_line_end-K%d" % _K, each(one(_gray_line_end(_K))),
         lambda: [Packed(cw.gray_levels(5))] + [noise(s + (1,), 600 + i) for i, s in enumerate(POINT_SHAPES)],
         max(2 * sum(h * w for h, w in cw.GRAY_EXTENTS), PX) * (1 + _K) * 4)

TINY = [((1, 1), 1), ((4, 9), 2), ((5, 5), 2), ((6, 70), 3), ((16, 56), 2), ((17, 57), 3), ((24, 224), 2), ((25, 225), 2)]


def _tiny(hw, n_levels):
    def calls(rt, f32, u8, u8x3):
        from pysilent_amd.util.zoom.from_image import classic_levels
        plan = plan_of(rt, ("tiny", hw), hw, 1, classic_levels(hw, 2.0, n_levels))
        cs_k, bank = _gray_weights(4)
        return [lambda: (plan.run(f32),), lambda: (plan.run(u8, frame_dtype="uint8"),),
                lambda: plan.gray_pass(f32, cs_k, bank),
                lambda: plan.gray_pass(u8, cs_k, bank, storage="float16", frame_dtype="uint8"),
                lambda: plan.gray_pass(u8x3, cs_k, bank, frame_dtype="uint8", frame_channels=3),
                lambda: gray_keypoints(rt, plan, f32, 4)]
    return calls


for _hw, _n in TINY:             # test_gray_pass_tiny_and_tile_boundary_frames
    case("tiny-%dx%d" % _hw, _tiny(_hw, _n), _plan_inputs(_hw, 1, 700 + _hw[1]), 2 * (2 * _hw[0] * _hw[1]) * (24 + 8 + 32) + 4096, workspace=True)


# ----------------------------------------------------------------------------- the RGB chain

RGB_KNOBS = (1, 2, 16, 64, 64 | 16, 128, 5 << 8)          # (5 << 8: 10-row tiles, bits 8-15 = tile height / 2)
STORE_PX = 2 * sum(h * w for h, w in cw.STORE_EXTENTS)
RGB_PX = max(max(n * h * w for n, h, w, _ in cw.RGB_SHAPES), STORE_PX)


def _rgb_line_end(name, policies, knob=0):
    def f(rt, x):
        from pysilent_amd._lib import TUNE_RGB
        ks = cw.rgb_weights(name)

        def run(policy):
            r = rt.rgb_line_end(x, ks, flat_policy=policy)
            return r["orient"], r["line_end"], r["value"]
        return [knobbed(rt, TUNE_RGB, knob, lambda p=p: run(p)) for p in policies]
    return f


def _rgb_inputs(with_store_levels):
    def make():
        xs = [cw.rgb_frames(s) for s in cw.RGB_SHAPES]
        return xs + ([Packed(cw.store_levels())] if with_store_levels else [])
    return make


for _name in cw.RGB_BUILDERS:
    case("rgb_line_end-%s" % _name, each(_rgb_line_end(_name, ("ieee", "zero"))), _rgb_inputs(False), RGB_PX * 28, workspace=_name == "nonuniform_blur")
    for _knob in RGB_KNOBS:
        case("rgb_line_end-%s-knob%d" % (_name, _knob), each(_rgb_line_end(_name, ("ieee",), _knob)), _rgb_inputs(_knob == 128), RGB_PX * 28,
             default_route=False)


def _chain_params(name, policy="ieee"):
    from pysilent_amd import _lib
    ks = {n: np.ascontiguousarray(np.asarray(cw.rgb_weights(name)[n], np.float64).astype(np.float32)) for n in cw.RGB_NAMES}
    fp = C.POINTER(C.c_float)
    prm = _lib.RgbChainParams(*[ks[n].ctypes.data_as(fp) for n in cw.RGB_NAMES], 1.0, 0.1, {"ieee": _lib.FLAT_IEEE, "zero": _lib.FLAT_ZERO}[policy],
                              255.0, 2)
    return prm, ks


def _regions(op, regions):
    from pysilent_amd import _lib
    if regions is None:
        regions = [(max(h // 2, 1), max(w // 2, 1)) for h, w in op.extents]
    return (_lib.Extent * op.n_levels)(*[_lib.Extent(int(a), int(b)) for a, b in regions])


def _call(op, overflow, name, *args):
    """op.call; with ``overflow`` the host form must answer SILENT_E_CAPACITY (the wrapper's ValueError), the device form cannot."""
    try:
        op.call(name, *args)
    except ValueError:
        assert overflow and not op.dev
        return
    assert not overflow or op.dev, "%s: a cap_per_frame below the count did not raise" % name


def _overflowed(counts, cap):
    """The case really asks for more rows than the buffer holds, in every frame."""
    assert (wc.to_numpy(counts) > cap).all(), (wc.to_numpy(counts), cap)


def rgb_keypoints(rt, x, name, regions=None, peak_value=True, cap=None, overflow=False, policy="ieee"):
    """silent_rgb_keypoints[_dev] through _Operand, as a wrapper would call it."""
    op = rt._Operand(x, channels=3)
    prm, keep = _chain_params(name, policy)
    cap = op.frame_px if cap is None else cap
    (orient, optr), (line, lptr), (value, vptr) = op.alloc(3), op.alloc(3), op.alloc(1)
    pv, pptr = op.alloc(1) if peak_value else (None, None)
    idx, iptr = op.empty((op.n_frames, cap, 4), np.int64)
    counts, cptr = op.empty(op.n_frames, np.int64)
    _call(op, overflow, "rgb_keypoints", op.ptr, *op.geom(), C.byref(prm), 0.1, _regions(op, regions), optr, lptr, vptr, pptr, iptr, cap, cptr)
    if overflow:
        _overflowed(counts, cap)
    return op.wrap(orient, 3), op.wrap(line, 3), op.wrap(value, 1), (op.wrap(pv, 1) if peak_value else None), wc.Rows(idx, counts)


def select_keypoints(rt, x, regions=None, peak_value=True, cap=None, overflow=False):
    op = rt._Operand(x)
    cap = op.frame_px if cap is None else cap
    pv, pptr = op.alloc(1) if peak_value else (None, None)
    idx, iptr = op.empty((op.n_frames, cap, 4), np.int64)
    counts, cptr = op.empty(op.n_frames, np.int64)
    _call(op, overflow, "select_keypoints", op.ptr, None, *op.geom(), op.c, 0.1, _regions(op, regions), pptr, iptr, cap, cptr)
    if overflow:
        _overflowed(counts, cap)
    return (op.wrap(pv, 1) if peak_value else None), wc.Rows(idx, counts)


def max_value_indices_region(rt, x, regions=None, cap=None, overflow=False):
    op = rt._Operand(x, channels=1)
    cap = op.frame_px if cap is None else cap
    idx, iptr = op.empty((op.n_frames, cap, 4), np.int64)
    counts, cptr = op.empty(op.n_frames, np.int64)
    _call(op, overflow, "max_value_indices_region", op.ptr, *op.geom(), _regions(op, regions), iptr, cap, cptr)
    if overflow:
        _overflowed(counts, cap)
    return (wc.Rows(idx, counts),)


def _rgb_keypoints(name, knob, policies=("ieee",)):
    """With and without the peak-value map (without: the map lives in the context workspace)."""
    def f(rt, x):
        from pysilent_amd._lib import TUNE_RGB
        return [knobbed(rt, TUNE_RGB, knob, lambda p=p, pv=pv: rgb_keypoints(rt, x, name, peak_value=pv, policy=p))
                for p in policies for pv in (True, False)]
    return f


KP_EXTENTS = [(70, 131), (35, 66), (18, 33)]
KP_PX = 2 * sum(h * w for h, w in KP_EXTENTS)


def _kp_pyramid():
    return [Packed([cw.rgb_frames((2, h, w, 3)) for h, w in KP_EXTENTS])]


for _name in cw.RGB_BUILDERS:
    case("rgb_keypoints-%s-sparse" % _name, each(_rgb_keypoints(_name, 0)), _kp_pyramid, KP_PX * 64 + 4096, workspace=True)
    case("rgb_keypoints-%s-dense" % _name, each(_rgb_keypoints(_name, 32)), _kp_pyramid, KP_PX * 64 + 4096, default_route=False, workspace=True)

# the chain of silent_rgb_keypoints is not that of silent_rgb_line_end (extrema, value summary and NaN flags as extra outputs; sparse or
# dense tail by kernel form): the wave / tile edge shapes and the knob list again, one fused class and the staged one, both policies
for _name in ("symmetric", "nonuniform_blur"):
    case("rgb_keypoints-%s-shapes" % _name, each(_rgb_keypoints(_name, 0, ("ieee", "zero"))), _rgb_inputs(False), RGB_PX * 64 + 4096, workspace=True)
    for _knob in RGB_KNOBS:
        case("rgb_keypoints-%s-shapes-knob%d" % (_name, _knob), each(_rgb_keypoints(_name, _knob, ("zero",))), _rgb_inputs(_knob == 128),
             RGB_PX * 64 + 4096, default_route=False, workspace=True)


def _many_windows():
    """test_select_keypoints_with_many_windows: plateaus, so that ties and whole windows of equal values occur."""
    rng = np.random.default_rng(3)
    return [Packed([np.floor(rng.random((2, h, w, 3)) * 8).astype(np.float32) * 32 for h, w in [(37, 131), (70, 60), (5, 7)]])]


def _select_keypoints(regions):
    return lambda rt, x: [lambda pv=pv: select_keypoints(rt, x, regions, peak_value=pv) for pv in (True, False)]


MW_PX = 2 * (37 * 131 + 70 * 60 + 35)
case("select_keypoints-few_windows", each(_select_keypoints(None)), _many_windows, MW_PX * 36 + 4096, workspace=True)
case("select_keypoints-many_windows", each(_select_keypoints([(3, 3)] * 3)), _many_windows, MW_PX * 36 + 4096, workspace=True)


def _value_maps():
    x = noise((2, 40, 40, 1), 8)
    x[0, :20, :20] = 0
    return [x, Packed([noise((2, h, w, 1), 9 + h) for h, w in [(37, 53), (19, 27), (5, 3)]])]


VM_PX = 2 * max(1600, 37 * 53 + 19 * 27 + 15)
case("max_value_indices_region-few_windows", each(one(lambda rt, x: max_value_indices_region(rt, x))), _value_maps, VM_PX * 32 + 4096, workspace=True)
case("max_value_indices_region-many_windows",
     each(lambda rt, x: [lambda r=r: max_value_indices_region(rt, x, [r] * len(rt._Operand(x).extents)) for r in ((3, 3), (1, 7))]),
     _value_maps, VM_PX * 32 + 4096, workspace=True)


# ----------------------------------------------------------------------------- index buffers smaller than the count

CAP = 10


def _zero_map(c):
    return lambda: [np.zeros((2, 16, 16, c), np.float32)]              # test_max_value_indices_capacity_error: 256 rows a frame


def _gray_keypoints_overflow(rt, f32, u8, u8x3):
    """A black frame: every pixel of every level is a keypoint (selection = 0)."""
    from pysilent_amd.util.zoom.from_image import classic_levels
    hw = (16, 56)
    plan = plan_of(rt, ("tiny", hw), hw, 1, classic_levels(hw, 2.0, 2))
    return [lambda: gray_keypoints(rt, plan, f32 * 0, 4, selection=False, cap=CAP, overflow=True)]


case("overflow-max_value_indices_region", each(one(lambda rt, x: max_value_indices_region(rt, x, [(8, 8)], cap=CAP, overflow=True))), _zero_map(1),
     2 * CAP * 32 + 4096)
case("overflow-select_keypoints", each(one(lambda rt, x: select_keypoints(rt, x, [(8, 8)], cap=CAP, overflow=True))), _zero_map(3),
     2 * (CAP * 32 + 1024) + 4096)
# (flat policy "zero": a black frame gives an all-zero line-end map, not the NaNs of 0 * inf, so every pixel is a keypoint)
case("overflow-rgb_keypoints",
     each(lambda rt, x: [lambda pv=pv: rgb_keypoints(rt, x, "symmetric", [(8, 8)], peak_value=pv, cap=CAP, overflow=True, policy="zero") for pv in (True, False)]),
     _zero_map(3), 2 * (CAP * 32 + 256 * 32) + 4096)
case("overflow-gray_keypoints", _gray_keypoints_overflow, _plan_inputs((16, 56), 1, 800), 2 * 16 * 56 * 2 * 32 + 2 * CAP * 32 + 4096)

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)
