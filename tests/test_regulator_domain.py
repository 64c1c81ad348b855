"""CPU side of tests/test_gpu_regulator_domain.py: the divisive regulator y = x * rv / pow(min(blur(x), 1), root) over the blur's
whole range, from above 1 down to the denormals.

  * cw.rgb_dyadic() is detected as the symmetric class and every kernel form streams its weights back EXACTLY;
  * on cw.exact_frames() stripe and blur are exact in float32 (the premise: every partial sum is an integer below 2^24 units), at
    k = 0 and with the unit dimmed to the smallest denormal -- so the only inexact operations left in orient are the regulator's;
  * the dimming sweep of the GPU test (cw.dimmed(cw.param_frames(), k)) is attainable by torch's float32 evaluation, every class;
  * the sharp assertion (cw.assert_regulator_sharp, allowance derived in cw.regulator_allowance) is attainable by a float32 model of
    both regulator paths and raises for six ways a kernel could get the regulator wrong.

Why this file exists: the first of those six, a factor that is off by 4e-6, passes the end-to-end assert_close(..., bound=...) of
the chain tests (last assertion of the sensitivity test), because that bound carries the blur's own uncertainty."""
import numpy as np
import pytest

import chain_weights as cw
import err_bound as eb
import silent_oracle as so
from test_chain_weights import _check_rgb_case, _lib_or_skip, _raises, _walk_stream

POLICIES = ("zero", "ieee")
THRESHOLD = np.float32(7.8886e-31)        # below it (and above 0) the fused kernels take powf and a true division
EXACT_ROOTS = cw.PRESCRIBED_ROOTS


def exact_chain(k, root, rv, policy):
    """The oracle on the dimmed exact frames, and m = min(blur, 1) of its (exact) stripe."""
    ks, x = cw.rgb_dyadic(), cw.dimmed(cw.exact_frames(), k)
    want = so.rgb_line_end_chain(x, ks, policy, root, rv)
    b = so.conv2d_same(want["stripe"], ks["blur"])
    return want, np.minimum(b, np.float32(1.0))


# ----------------------------------------------------------------------------- class detection, exact streaming

def test_dyadic_weights_are_the_symmetric_class_and_stream_back_exactly():
    _lib_or_skip()
    from test_host_logic import _chain_stream, _chain_structure
    ks = cw.rgb_dyadic()
    flags, masks = _chain_structure(ks)
    assert flags == 0b111111 and masks == [cw.RGBY_MASK] * 3 + list(cw.END_MASKS)
    for knob, var in ((0, 3), (64, 2), (2, 1), (1, 0)):
        stream, n, variant, a = _chain_stream(ks, knob)
        assert variant == var
        _walk_stream(stream, n, variant, a, masks, exact=True)
    for name in cw.RGB_NAMES:                    # small dyadic numbers: float32 holds them as they are
        np.testing.assert_array_equal(ks[name].astype(np.float32).astype(np.float64), ks[name])
        unit = {"blur": 8.0, "end": 64.0, "rgby": 16.0}.get(name, 4.0)
        np.testing.assert_array_equal(np.round(ks[name] * unit), ks[name] * unit)


# ----------------------------------------------------------------------------- the exactness premise

def _front32(x, ks):
    """stripe and blur by torch's float32 convolutions: another summation order than the oracle's float64 one."""
    import torch
    F = torch.nn.functional

    def conv(t, k):
        kt = torch.from_numpy(np.asarray(k, np.float64).astype(np.float32)).permute(3, 2, 0, 1)
        p = (kt.shape[-1] - 1) // 2
        return F.conv2d(F.pad(t, (p, p, p, p)), kt)

    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    stripe = torch.relu(conv(torch.relu(conv(torch.relu(conv(t, ks["rgc"])), ks["rgby"])), ks["stripe"]))
    return stripe.permute(0, 2, 3, 1).numpy(), conv(stripe, ks["blur"]).permute(0, 2, 3, 1).numpy()


def test_every_partial_sum_on_the_exact_frames_is_an_integer_below_2_to_24_units():
    """A condition of the inputs (seed cw.DYADIC_SEED): sum |w| |x| per stage, in units of the stage's output, bounds every
    partial sum in every order and regrouping; the factored forms' inner sums (S . x before the mix, x + x' before a shared tap)
    have coarser units and are bounded by sum |x| of the stage's window."""
    ks, x = cw.rgb_dyadic(), cw.exact_frames()
    assert 0.03 * 0.6 < (x != 0).any(-1).mean() < 0.06 and x.max() == 3 and not x[0, 8:28, 20:50].any()
    want = so.rgb_line_end_chain(x, ks, "zero")
    maps = dict(frame=x, rgc=want["rgc"], rgby=want["rgby"], stripe=want["stripe"], blur=so.conv2d_same(want["stripe"], ks["blur"]))
    for src, name in (("frame", "rgc"), ("rgc", "rgby"), ("rgby", "stripe"), ("stripe", "blur")):
        unit, unit_in = 2.0 ** cw.EXACT_UNIT_LOG2[name], 2.0 ** cw.EXACT_UNIT_LOG2[src]
        k32 = np.asarray(ks[name], np.float32).astype(np.float64)
        sums = eb._corr_same(np.abs(maps[src]), np.abs(k32)) / unit
        window = eb._corr_same(np.abs(maps[src]), np.ones_like(k32)) / unit_in
        assert sums.max() < 2.0 ** 24 and window.max() < 2.0 ** 24, (name, sums.max(), window.max())
        got = np.asarray(maps[name], np.float64) / unit
        np.testing.assert_array_equal(got, np.round(got), err_msg=name)
    assert (maps["blur"] > 0).mean() > 0.8 and (maps["blur"] >= 1).mean() > 0.5


@pytest.mark.parametrize("k", [0, cw.EXACT_K_UNIT_AT_2M149])
def test_stripe_and_blur_of_the_exact_frames_are_exact_in_float32(k):
    pytest.importorskip("torch")
    ks, x = cw.rgb_dyadic(), cw.dimmed(cw.exact_frames(), k)
    want = so.rgb_line_end_chain(x, ks, "zero")
    blur = so.conv2d_same(want["stripe"], ks["blur"])
    stripe32, blur32 = _front32(x, ks)
    np.testing.assert_array_equal(stripe32.view(np.int32), want["stripe"].view(np.int32))
    np.testing.assert_array_equal(blur32.view(np.int32), blur.view(np.int32))
    # and they are the k = 0 maps times 2^-k: fixed-point multiples of the unit, down to the smallest denormal
    base = so.rgb_line_end_chain(cw.exact_frames(), ks, "zero")
    np.testing.assert_array_equal(blur.astype(np.float64), so.conv2d_same(base["stripe"], ks["blur"]).astype(np.float64) * 2.0 ** -k)
    if k:
        pos = blur[blur > 0]
        assert pos.min() >= 2.0 ** -149 and pos.max() < 2.0 ** -126          # all of it denormal


# ----------------------------------------------------------------------------- attainability of the dimming sweep

@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", sorted(cw.RGB_BUILDERS))
def test_float32_evaluation_meets_the_dimming_sweep(name, policy):
    pytest.importorskip("torch")
    ks = cw.rgb_weights(name)
    for k in cw.DIM_K:
        x = cw.dimmed(cw.param_frames(), k)
        for root in cw.DIM_ROOTS:
            _check_rgb_case(name, ks, x, policy, (1.0, root, 255.0, 2), "%s %s k %d root %g" % (name, policy, k, root))


# ----------------------------------------------------------------------------- the sharp assertion: attainable, and it bites

def regulator32(x, b, rv, root, policy, fused, mutation=None):
    """A float32 model of the regulator on an exact stripe x and blur b: the per-op kernels' form (powf, a division) or the fused
    kernels' (rv * exp2(-root * log2 m); powf and a division for 0 < m < THRESHOLD and for root == 0).  powf is modelled by the
    correctly rounded power, log2 / exp2 by NumPy's float32 ones.  ``mutation``: one way to get it wrong."""
    x, b = np.asarray(x, np.float32), np.asarray(b, np.float32)
    rv32 = np.float32(rv)
    root32 = np.float32(np.float16(root)) if mutation == "float16 root" else np.float32(root)
    m = b if mutation == "no min" else np.where(b > 1, np.float32(1), b).astype(np.float32)
    if mutation == "below 2^-100 is 0":
        m = np.where(m < np.float32(2.0 ** -100), np.float32(0), m)
    if mutation == "denormal is 0":
        m = np.where(np.abs(m) < np.float32(2.0 ** -126), np.float32(0), m)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r_pow = rv32 / np.power(m.astype(np.float64), np.float64(root32)).astype(np.float32)
        log = np.log(m) if mutation == "natural log" else np.log2(m)
        r_exp = rv32 * np.exp2((-root32 * log).astype(np.float32)).astype(np.float32)
        slow = ((m > 0) & (m < THRESHOLD)) | (root32 == 0) | (not fused)
        r = np.where(slow, r_pow, r_exp).astype(np.float32)
        if mutation == "factor 4e-6":
            r = (r * np.float32(1 + 4e-6)).astype(np.float32)
        y = (x * r).astype(np.float32)
    return np.where(x == 0, np.float32(0), y).astype(np.float32) if policy == "zero" else y


def exact_cases():
    """(k, root) of the sharp tests.  t = root * |log2 m| <= 120 wherever orient is finite and non-zero keeps the oracle's power a
    normal float32: root 1 stops at k = 120 (the smallest blur under a non-zero stripe is 2^2.9 * 2^-k)."""
    return [(k, root) for root in EXACT_ROOTS for k in cw.EXACT_K if root * (k - 2) <= 120]


def test_the_exact_cases_cover_the_blurs_ranges():
    want, m = exact_chain(0, 0.1, 1.0, "zero")
    b = so.conv2d_same(want["stripe"], cw.rgb_dyadic()["blur"])
    on = np.log2(b[want["stripe"] > 0].astype(np.float64))
    lo, hi = on.min(), on.max()
    assert 2 < lo < 3 and 6 < hi < 7 and np.log2(b[b > 0].min()) < -7, (lo, hi)
    at = {k: (lo - k, hi - k) for k in cw.EXACT_K}
    assert at[5][0] < 0 < at[5][1] and at[105][0] < -100 < at[105][1]                # across 1, across 2^-100 (the kernels' threshold)
    assert abs(at[45][0] + 40) < 5 and abs(at[85][0] + 80) < 5
    assert -126 < at[120][0] and at[120][1] < -101                                   # inside the powf branch, normal
    assert at[131][0] < -126 < at[131][1] and at[138][1] < -126 and lo - 138 > -149  # across FLT_MIN, all denormal
    assert {(105, 1.0), (120, 1.0), (131, 0.5), (138, 0.5), (138, 0.0)} <= set(exact_cases()) and (131, 1.0) not in exact_cases()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("fused", [False, True])
def test_float32_model_of_the_regulator_meets_the_sharp_assertion(fused, policy):
    for k, root in exact_cases():
        for rv in cw.DIM_RVS:
            want, m = exact_chain(k, root, rv, policy)
            b = so.conv2d_same(want["stripe"], cw.rgb_dyadic()["blur"])
            got = regulator32(want["stripe"], b, rv, root, policy, fused)
            cw.assert_regulator_sharp(got, want["orient"], m, root, fused, "model k %d root %g rv %g %s" % (k, root, rv, policy))


# mutation -> (k, root) at which it must show: (blur across 1 / across 2^-100 / all denormal)
MUTATIONS = {"factor 4e-6": (5, 0.1), "below 2^-100 is 0": (105, 0.5), "denormal is 0": (138, 0.5), "no min": (5, 0.5),
             "float16 root": (45, 0.1), "natural log": (45, 0.5)}


@pytest.mark.parametrize("policy", POLICIES)
def test_the_sharp_assertion_sees_six_wrong_regulators(policy):
    for mutation, (k, root) in MUTATIONS.items():
        want, m = exact_chain(k, root, 1.0, policy)
        b = so.conv2d_same(want["stripe"], cw.rgb_dyadic()["blur"])
        cw.assert_regulator_sharp(regulator32(want["stripe"], b, 1.0, root, policy, True), want["orient"], m, root, True, "unmutated")
        bad = regulator32(want["stripe"], b, 1.0, root, policy, True, mutation)
        with pytest.raises(AssertionError):
            cw.assert_regulator_sharp(bad, want["orient"], m, root, True, mutation)
    # ... and why the end-to-end assertion of the chain tests is not enough: the factor off by 4e-6 is inside its bound, on these
    # frames at every k and root, since that bound carries the uncertainty a float32 blur would have
    ks = cw.rgb_dyadic()
    for k, root in exact_cases():
        if root == 0.0 or k > 120:           # (root 0 has no factor; below 2^-126 assert_close's own 1e-38 hides everything)
            continue
        x = cw.dimmed(cw.exact_frames(), k)
        want, m = exact_chain(k, root, 1.0, policy)
        bound = eb.rgb_chain(x, ks, want, policy, root, 1.0)
        b = so.conv2d_same(want["stripe"], ks["blur"])
        bad = regulator32(want["stripe"], b, 1.0, root, policy, True, "factor 4e-6")
        assert not np.array_equal(bad, want["orient"])
        assert not _raises(bad, want["orient"], bound=bound["orient"]), (k, root)


@pytest.mark.parametrize("policy", POLICIES)
def test_float32_model_meets_the_per_op_assertions_on_prescribed_blur_values(policy):
    """Part C of the GPU test with the powf model in the kernels' place: 0, -0, denormals, FLT_MIN, both sides of the fused kernels'
    threshold and of 2^-100, 1 -+ ulp, FLT_MAX, inf, NaN and negative blurs are all inside the powf allowance or of the oracle's class."""
    def model(mutation=None):
        def regulate(x, blur, rv, root):
            with np.errstate(invalid="ignore"):          # (0 * inf around the inf pixel)
                return regulator32(x, so.conv2d_same(x, blur), rv, root, policy, False, mutation)
        return regulate

    worst = {}
    cw.check_prescribed(model(), policy, worst)
    assert len(worst) >= 3 * 4 and max(worst.values()) <= 1.0
    with pytest.raises(AssertionError):          # ... and a kernel that flushed a denormal blur to 0 would be seen
        cw.check_prescribed(model("denormal is 0"), policy, {})
