"""The divisive regulator y = x * rv / pow(min(blur(x), 1), root) of every RGB chain form over its blur's whole range: from above 1
down to 2^-113 end to end on every weight class (A), on frames whose stripe and blur are EXACT in float32 held to the regulator's own
derived allowance down to the denormals (B), and the per-op regulate on prescribed blur values (C).  Five pieces of code evaluate
the regulator -- powf in conv2d_same_kernel<REG> / the generic conv kernel and in regulate_sum_kernel, rv * exp2(-root * log2 m) in
regulator_ratio (the one-pixel kernel, the non-symmetric pair forms), the same inlined in the symmetric pair form, and all of them
behind the float16 store path; the other chain tests keep the blur above 2^-14.  tests/test_regulator_domain.py shows on the CPU
that these assertions are attainable in float32 and which wrong regulators they catch.  Each test prints its worst |err| / allowance
(or bound) per form (pytest -s)."""
import numpy as np
import pytest

import chain_weights as cw
import err_bound as eb
import silent_oracle as so
from conftest import WORST_BOUND
from pysilent_amd._lib import TUNE_RGB
from test_regulator_domain import exact_cases, exact_chain

pytestmark = pytest.mark.gpu

POLICIES = ("zero", "ieee")
LADDER = {3: (0, 64, 2, 1), 2: (0, 2, 1), 1: (0, 1), 0: (0,)}      # SILENT_TUNE_RGB: each knob moves a class's weights one form down
FORM = {0: "symmetric", 64: "two-group", 2: "basic", 1: "dense"}


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _knobs(name):
    """(knob, label) of every kernel form these weights can run in: the pair kernel's ladder and, | 16, the one-pixel kernel's
    (which has no symmetric form: knob 16 runs its two-group one)."""
    if name not in cw.RGB_VARIANTS:
        return [(0, "staged")]
    variant = cw.RGB_VARIANTS[name][0]
    pair = [(kn, ("dense", "basic", "two-group", "symmetric")[variant] if kn == 0 else FORM[kn]) for kn in LADDER[variant]]
    one = [(kn | 16, "two-group (knob 16)" if form == "symmetric" else form) for kn, form in pair]
    return [(kn, "pair " + form) for kn, form in pair] + [(kn, "one-pixel " + form) for kn, form in one]


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), "%s: NaN pattern differs" % what
    bits = np.uint32 if a.dtype == np.float32 else np.uint16
    np.testing.assert_array_equal(a[~nan].view(bits), b[~nan].view(bits), err_msg=what)


def _assert_rounded(h, f, what):
    """h: the float16 map, f: the float32 map it must be the rounding of (nearest even, overflow to inf, subnormals kept)."""
    h, f = np.asarray(h), np.asarray(f)
    assert h.dtype == np.float16 and f.dtype == np.float32, what
    with np.errstate(over="ignore"):
        _same_bits(h, f.astype(np.float16), what)


# ----------------------------------------------------------------------------- A. dimming sweep, end to end

class _Front(object):
    """The oracle's maps before the regulator and their bounds for one (class, k): shared by the 12 (policy, root, rv) of a sweep."""

    def __init__(self, ks, x):
        self.ks = ks
        self.rgc = so.conv2d_same(x, ks["rgc"], relu=True)
        self.rgby = so.conv2d_same(self.rgc, ks["rgby"], relu=True)
        self.stripe = so.conv2d_same(self.rgby, ks["stripe"], relu=True)
        e_rgc = eb.conv(x, ks["rgc"])
        e_rgby = eb.conv(self.rgc, ks["rgby"], e_rgc)
        self.e_stripe = eb.conv(self.rgby, ks["stripe"], e_rgby)

    def tail(self, policy, root, rv, clip=255.0, pad=2):
        """(want, bound) as so.rgb_line_end_chain and eb.rgb_chain give them (the first test compares)."""
        ks = self.ks
        orient = so.regulate(self.stripe, ks["blur"], rv, root, policy)
        line_end = so.conv2d_same(orient, ks["end"], relu=True, clip_hi=clip)
        padded = so.pad_inwards(line_end, [[0, 0], [pad, pad], [pad, pad], [0, 0]])
        want = dict(orient=orient, line_end=line_end, padded=padded, value=so.value_from_color(padded))
        e = dict(orient=eb.regulate(self.stripe, ks["blur"], rv, root, self.e_stripe, policy))
        if policy == "ieee":
            e["orient"] = np.where(np.isnan(orient), eb.BIG, e["orient"])
        e["padded"] = eb.pad(eb.conv(orient, ks["end"], e["orient"]), pad)
        e["value"] = eb.value(padded, e["padded"])
        return want, e


def test_the_shared_front_is_the_oracles_chain():
    ks, x = cw.rgb_weights("symmetric"), cw.dimmed(cw.param_frames(), 70)
    want, e = _Front(ks, x).tail("ieee", 0.5, 0.7)
    ref = so.rgb_line_end_chain(x, ks, "ieee", 0.5, 0.7)
    ref_e = eb.rgb_chain(x, ks, ref, "ieee", 0.5, 0.7)
    for name in ("orient", "padded", "value"):
        np.testing.assert_array_equal(want[name], ref[name])
        np.testing.assert_array_equal(e[name], ref_e[name])


def _worst_of(tag):
    return max([v[0] for k, v in WORST_BOUND.items() if k.endswith(tag)] or [0.0])


@pytest.mark.parametrize("name", sorted(cw.RGB_BUILDERS))
def test_dimming_sweep_against_the_oracle(rt, name):
    """cw.dimmed(cw.param_frames(), k), k = 0 .. 110 (noise and a line drawing: exact zeros), roots 0.1 / 0.5 / 1, rv 1 / 0.7, both
    flat policies, every kernel form of the class: a wrong branch, a flush or an overflow anywhere between 2^-113 and 1 fails the
    project's end-to-end assertions (NaN pattern, infinities, 1e-5 range-relative, the element-wise bound).  The float16 entry
    point (fused classes, default form): the float32 maps of the same form rounded once, the value map bit for bit."""
    ks = cw.rgb_weights(name)
    forms = _knobs(name)
    worst = {}
    try:
        for k in cw.DIM_K:
            x = cw.dimmed(cw.param_frames(), k)
            front = _Front(ks, x)
            for policy in POLICIES:
                for root in cw.DIM_ROOTS:
                    for rv in cw.DIM_RVS:
                        want, bound = front.tail(policy, root, rv)
                        got = {}
                        for knob, form in forms:
                            tag = "sweep %s %s" % (name, form)
                            with rt.tuning(TUNE_RGB, knob):
                                got[knob] = rt.rgb_line_end(x, ks, regulation_value=rv, regulation_root=root, flat_policy=policy)
                            try:
                                cw.assert_rgb_chain_close(got[knob], want, bound, 255.0, tag)
                            except AssertionError as e:
                                raise AssertionError("k %d root %g rv %g %s: %s" % (k, root, rv, policy, e))
                            worst[form] = _worst_of(tag)
                        if name in cw.RGB_VARIANTS and rv == 0.7:
                            half = rt.rgb_line_end(x, ks, regulation_value=rv, regulation_root=root, flat_policy=policy, storage="float16")
                            tag = "float16 %s k %d root %g %s" % (name, k, root, policy)
                            _assert_rounded(half["orient"], got[0]["orient"], "orient " + tag)
                            _assert_rounded(half["line_end"], got[0]["line_end"], "line_end " + tag)
                            _same_bits(half["value"], got[0]["value"], "value " + tag)
    finally:
        print("\ndimming sweep %s: worst |err| / bound per form: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["symmetric", "two_group", "basic_blur", "dense", "nonuniform_blur"])
def test_fused_keypoints_on_dimmed_frames_equal_chain_then_selection(rt, name, policy):
    """silent_rgb_keypoints on cw.dimmed(cw.pipeline_frames(), 70) (maps around 2^-60, a NaN and an inf pixel) against
    silent_rgb_line_end + silent_select_keypoints on the same pyramid: maps and keypoints bit for bit."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline
    ks = cw.rgb_weights(name)
    hw = cw.PIPELINE_HW
    frames = cw.dimmed(cw.pipeline_frames(), 70)
    common = dict(mode="rgb", n_levels=4, batch=3, selection=True, max_keypoints_per_frame=1 << 16, flat_policy=policy, constants=ks)
    fused, plain = LineEndPipeline(hw, **common), LineEndPipeline(hw, **common)
    t = torch.from_numpy(frames).cuda()
    fused.step(t)
    plain.run_pyramid(t)
    plain.run_filters()
    plain.run_keypoints()
    torch.cuda.synchronize()
    a, b = fused.outputs(), plain.outputs()
    for m in ("orient", "line_end", "value", "peak_value"):
        _same_bits(a[m].data.cpu().numpy(), b[m].data.cpu().numpy(), "%s %s" % (name, m))
    np.testing.assert_array_equal(a["keypoint_counts"], b["keypoint_counts"])
    for f in range(3):
        np.testing.assert_array_equal(a["keypoints"][f], b["keypoints"][f])
    assert sum(len(k) for k in a["keypoints"]) > 0
    v = a["value"].level(0)[0].cpu().numpy()
    assert 0 < np.nanmax(v) < 2.0 ** -40             # the maps the keypoints come from are really dim


# ----------------------------------------------------------------------------- B. exact frames, sharp

@pytest.mark.parametrize("policy", POLICIES)
def test_exact_frames_hold_the_regulators_own_allowance(rt, policy):
    """cw.rgb_dyadic() on cw.dimmed(cw.exact_frames(), k): the blur across 1, near 2^-40 and 2^-80, across 2^-100 (below it the fused
    kernels take powf), inside [2^-126, 2^-101], across 2^-126 and in the denormals; roots 0 / 0.1 / 0.5 / 1, rv 1 / 0.7.  The symmetric
    class on its knob ladder and the one-pixel kernel.  First the stripe (orient with root 0, rv 1) is the oracle's bit for bit in every
    form; then orient is held, element by element, to cw.regulator_allowance -- (3 ln2 t + 8) * 2^-24 * |y| on the exp2 / log2 path,
    8 * 2^-24 * |y| on the powf path -- with 0, inf and NaN by class; the forms that share regulator_ratio are bit-identical; the
    float16 entry point stores the symmetric form's float32 orient rounded once."""
    ks = cw.rgb_dyadic()
    forms = _knobs("symmetric")
    worst = {}
    try:
        for k in cw.EXACT_K:
            x = cw.dimmed(cw.exact_frames(), k)
            want0, _ = exact_chain(k, 0.0, 1.0, policy)
            np.testing.assert_array_equal(want0["orient"].view(np.int32), want0["stripe"].view(np.int32))
            for knob, form in forms:
                with rt.tuning(TUNE_RGB, knob):
                    got = rt.rgb_line_end(x, ks, regulation_value=1.0, regulation_root=0.0, flat_policy=policy, want=("orient",))
                _same_bits(got["orient"], want0["stripe"], "stripe k %d %s" % (k, form))
        for k, root in exact_cases():
            x = cw.dimmed(cw.exact_frames(), k)
            for rv in cw.DIM_RVS:
                want, m = exact_chain(k, root, rv, policy)
                got = {}
                for knob, form in forms:
                    with rt.tuning(TUNE_RGB, knob):
                        got[knob] = np.asarray(rt.rgb_line_end(x, ks, regulation_value=rv, regulation_root=root, flat_policy=policy,
                                                               want=("orient",))["orient"])
                    cw.assert_regulator_sharp(got[knob], want["orient"], m, root, True, "orient k %d root %g rv %g %s" % (k, root, rv, form),
                                              worst, form)
                for knob, form in forms[2:]:         # (forms[0] is the symmetric pair form with its own inlined regulator)
                    _same_bits(got[knob], got[forms[1][0]], "regulator_ratio forms k %d root %g rv %g: %s vs %s" % (k, root, rv, form, forms[1][1]))
                half = rt.rgb_line_end(x, ks, regulation_value=rv, regulation_root=root, flat_policy=policy, want=("orient",), storage="float16")
                _assert_rounded(half["orient"], got[0], "float16 orient k %d root %g rv %g" % (k, root, rv))
    finally:
        cw.print_worst("exact frames, %s: worst |err| / allowance per form and range of m = min(blur, 1)" % policy, worst)


# ----------------------------------------------------------------------------- C. per-op regulate on prescribed blur values

@pytest.mark.parametrize("policy", POLICIES)
def test_per_op_regulate_on_prescribed_blur_values(rt, policy):
    """rt.regulate with a centre-delta blur, so the blur IS the pixel: 0 and -0, the smallest and largest denormal, FLT_MIN, the floats
    on both sides of 7.8886e-31 and of 2^-100, 1 -+ ulp, FLT_MAX, inf, NaN, -0.5 and -2.  A per-channel 7 x 7 delta
    (conv2d_same_kernel<7, 7, 3, 3, REG>), a per-channel 5 x 5 one (the generic conv kernel) and a channel-uniform 7 x 7 one
    (regulate_sum_kernel: the other two channels of each pixel are 0, so the channel sum is the pixel).  All three use powf and a
    division: 8 * 2^-24 * |y| against so.regulate, 0 / inf / NaN by class.  A negative blur follows powf like the oracle follows pow:
    NaN for roots 0.1 and 0.5, rv / b for root 1, rv for root 0 (include/silent_hip.h, silent_regulate)."""
    worst = {}
    try:
        cw.check_prescribed(lambda x, blur, rv, root: rt.regulate(x, blur, rv, root, policy), policy, worst)
    finally:
        cw.print_worst("per-op regulate, %s: worst |err| / allowance per kernel and range of m" % policy, worst)
