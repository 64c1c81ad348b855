"""Deterministic weights for the two fused chains that are GENERIC inside the structure class one kernel form is selected by
(test infrastructure, like tests/err_bound.py).

The reference's own constant kernels are very symmetric: rgc, rgby, the blur and the gray centre-surround kernel equal their
transpose, both flips and (where it applies) their C_in <-> C_out swap; the stripe bank equals its 180-degree rotation.  A fused
kernel that swaps dy and dx, mirrors a row, exchanges i and o, folds the blur over the wrong axis or uses channel 0's rgc profile
for every channel returns bit-identical maps on them.  The builders below start from the product's generators (so magnitudes
and conditioning stay in the class the response tolerance is stated for), jitter every free parameter of a class on its own
-- k * (1 + 0.3 * U(-1, 1)) -- and leave equal only what the class forces to be equal.  Structured kernels are float64
products, rounded to float32 once by whoever consumes them, as the generators' are.

Every builder returns float64 HWIO arrays and is a pure function of its seed.
"""
import numpy as np

AMP = 0.3            # jitter amplitude
FILL = 0.05          # dense fill, as a share of a kernel's largest weight
END_MASKS = (0x1f9, 0x119, 0x11f)       # group-A tap masks the two-group chain kernel is compiled for (bit t = dy * 3 + dx)
RGBY_MASK = 0x010

RGB_NAMES = ("rgc", "rgby", "stripe", "blur", "end")

_REF = {}


def reference():
    """The reference's kernels from the product generators, as the ``kernels`` fixture of conftest.py builds them."""
    if not _REF:
        from pysilent_amd import constant_convolutions as cc
        from pysilent_amd.util.normalize import normalize_tensor_positive_negative
        k = dict(rgc=cc.midget_rgc(2), rgby=cc.rgby_3(2), stripe=cc.rgb_2d_stripe_tensors(), blur=cc.blur_tensor(2, 7),
                 end=cc.rgb_2d_end_tensors(),
                 cs_gray=normalize_tensor_positive_negative(cc.center_surround_tensor(2, [1], [1], [1], [-1])),
                 end4=cc.end_bank(4), end8=cc.end_bank(8), end3=cc.end_bank(3))
        _REF.update({n: np.array(v, np.float64) for n, v in k.items()})
    return {n: v.copy() for n, v in _REF.items()}


def _rng(seed, tag):
    return np.random.default_rng([int(seed), sum(ord(c) * 131 ** i for i, c in enumerate(tag)) % (1 << 31)])


def _jit(rng, k, amp=AMP):
    k = np.asarray(k, np.float64)
    return k * (1.0 + amp * rng.uniform(-1.0, 1.0, k.shape))


def _fill(rng, k, share=FILL):
    """Every zero weight gets a value of its own: +- (0.5 ... 1) * share * the kernel's largest weight."""
    k = np.array(k, np.float64)
    f = share * np.abs(k).max() * rng.uniform(0.5, 1.0, k.shape) * rng.choice([-1.0, 1.0], k.shape)
    return np.where(k == 0, f, k)


# ----------------------------------------------------------------------------- pieces

def _rgc_symmetric(rng, ref):
    """Diagonal; per channel its own (corner, edge_h, edge_v, centre)."""
    k = np.zeros((3, 3, 3, 3))
    for c in range(3):
        r = ref["rgc"][:, :, c, c]
        co, eh, ev, ce = _jit(rng, [r[0, 0], r[0, 1], r[1, 0], r[1, 1]])
        k[:, :, c, c] = [[co, eh, co], [ev, ce, ev], [co, eh, co]]
    return k


def _rgc_diagonal(rng, ref):
    """Diagonal; per channel 9 taps of their own."""
    k = np.zeros((3, 3, 3, 3))
    for c in range(3):
        k[:, :, c, c] = _jit(rng, ref["rgc"][:, :, c, c])
    return k


def _rgby_mix(rng, ref):
    """S (x) A around the centre + B at the centre: S mirror-symmetric with corner != edge_v != edge_h, A and B full."""
    r = ref["rgby"]
    A = _fill(rng, _jit(rng, r[0, 0]), 0.3)
    B = _fill(rng, _jit(rng, r[1, 1]))
    ratio = float(np.abs(r[0, 1]).max() / np.abs(r[0, 0]).max())      # the reference's edge : corner
    eh, ev = _jit(rng, [ratio, ratio])
    S = np.array([[1.0, eh, 1.0], [ev, 0.0, ev], [1.0, eh, 1.0]])
    k = S[:, :, None, None] * A[None, None]
    k[1, 1] = B
    return k


def _rgby_two_group(rng, ref):
    """Per input channel: 8 surround taps that are distinct multiples of one vector, and a centre vector of its own."""
    r = ref["rgby"]
    A = _fill(rng, _jit(rng, r[0, 0]), 0.3)
    B = _fill(rng, _jit(rng, r[1, 1]))
    ratio = float(np.abs(r[0, 1]).max() / np.abs(r[0, 0]).max())
    k = np.zeros((3, 3, 3, 3))
    for i in range(3):
        prof = np.array([[1.0, ratio, 1.0], [ratio, 0.0, ratio], [1.0, ratio, 1.0]])
        k[:, :, i, :] = _jit(rng, prof)[:, :, None] * A[i][None, None]
        k[1, 1, i] = B[i]
    return k


def _stripe_sum(rng, ref):
    """Independent of the input channel (a filter of the channel sum): 27 values."""
    return np.repeat(_jit(rng, ref["stripe"][:, :, :1, :]), 3, axis=2)


def _centre_one(b):
    b[3, 3] = 1.0            # the regulator's own tap stays 1 (blur >= stripe: conftest.assert_regulated_close relies on it)
    return b


def _blur_folded(rng, ref):
    """Channel-uniform, mirror-symmetric in both axes, NOT a function of the distance: 16 values q[|dy|][min(dx, 6 - dx)]."""
    q = _jit(rng, ref["blur"][3:, :4, 0, 0])
    b = np.zeros((7, 7))
    for dy in range(7):
        for dx in range(7):
            b[dy, dx] = q[abs(dy - 3), min(dx, 6 - dx)]
    return np.repeat(np.repeat(_centre_one(b)[:, :, None, None], 3, 2), 3, 3)


def _blur_uniform(rng, ref):
    """Channel-uniform, 49 taps of their own."""
    b = _centre_one(_jit(rng, ref["blur"][:, :, 0, 0]))
    return np.repeat(np.repeat(b[:, :, None, None], 3, 2), 3, 3)


def _blur_per_channel(rng, ref):
    """A blur of its own per (i, o)."""
    return _jit(rng, ref["blur"])


def _end_two_group(rng, ref, masks=END_MASKS):
    """Per input channel: the taps of ``masks[i]`` are multiples of mixA[i], the others of mixB[i]; 9 scales of their own."""
    e = ref["end"].reshape(9, 3, 3)
    ref_masks = END_MASKS
    k = np.zeros((9, 3, 3))
    for i in range(3):
        tb = [t for t in range(9) if not ref_masks[i] >> t & 1]
        ref_a, ref_b = e[4, i], e[tb[0], i]
        mix_a, mix_b = _jit(rng, ref_a), _jit(rng, ref_b)
        for t in range(9):
            in_a_ref = bool(ref_masks[i] >> t & 1)
            base = ref_a if in_a_ref else ref_b
            j = int(np.argmax(np.abs(base)))
            scale = float(_jit(rng, e[t, i, j] / base[j]))
            k[t, i] = scale * (mix_a if masks[i] >> t & 1 else mix_b)
    return k.reshape(3, 3, 3, 3)


def _dense(rng, k):
    k = _jit(rng, k)
    return k + FILL * np.abs(k).max() * rng.uniform(0.5, 1.0, k.shape) * rng.choice([-1.0, 1.0], k.shape)


# ----------------------------------------------------------------------------- builders

def rgb_symmetric(seed):
    """Variant 3 (the symmetric forms of csrc/silent_rgb2.h)."""
    rng, ref = _rng(seed, "rgb_symmetric"), reference()
    return dict(rgc=_rgc_symmetric(rng, ref), rgby=_rgby_mix(rng, ref), stripe=_stripe_sum(rng, ref), blur=_blur_folded(rng, ref),
                end=_end_two_group(rng, ref))


def rgb_two_group(seed):
    """Variant 2: rgc without the mirror symmetry, an rgby surround that is not one profile; still two-group with the compiled masks."""
    rng, ref = _rng(seed, "rgb_two_group"), reference()
    return dict(rgc=_rgc_diagonal(rng, ref), rgby=_rgby_two_group(rng, ref), stripe=_stripe_sum(rng, ref), blur=_blur_folded(rng, ref),
                end=_end_two_group(rng, ref))


BASIC_FLAVOURS = ("blur", "masks", "dense")


def rgb_basic(seed, flavour="blur"):
    """Variant 1 (diagonal rgc + channel-sum stripe, everything else dense).  Flavours: "blur" -- the two-group weights with a
    uniform blur that is not mirror-symmetric; "masks" -- a two-group end bank whose masks are not the compiled ones (those of
    input channels 0 and 1 exchanged); "dense" -- dense rgby and end bank."""
    rng, ref = _rng(seed, "rgb_basic_" + flavour), reference()
    k = dict(rgc=_rgc_diagonal(rng, ref), rgby=_rgby_two_group(rng, ref), stripe=_stripe_sum(rng, ref), blur=_blur_folded(rng, ref),
             end=_end_two_group(rng, ref))
    if flavour == "blur":
        k["blur"] = _blur_uniform(rng, ref)
    elif flavour == "masks":
        k["end"] = _end_two_group(rng, ref, (END_MASKS[1], END_MASKS[0], END_MASKS[2]))
    elif flavour == "dense":
        k["rgby"], k["end"] = _dense(rng, ref["rgby"]), _dense(rng, ref["end"])
    else:
        raise KeyError(flavour)
    return k


def rgb_dense(seed):
    """Variant 0: every one of the 4 x 81 weights non-zero and of its own; a uniform blur with 49 taps of their own."""
    rng, ref = _rng(seed, "rgb_dense"), reference()
    k = {n: _dense(rng, ref[n]) for n in ("rgc", "rgby", "stripe", "end")}
    k["blur"] = _blur_uniform(rng, ref)
    return k


def rgb_nonuniform_blur(seed):
    """A blur that differs per (i, o): the staged path (workspace temporaries) instead of the fused launch."""
    rng, ref = _rng(seed, "rgb_nonuniform_blur"), reference()
    k = rgb_two_group(seed)
    k["blur"] = _blur_per_channel(rng, ref)
    return k


def gray_cs(seed):
    """[3,3,1,1]: 9 taps of their own, renormalised so that the positive taps sum to 1 and the negative ones to -1."""
    from pysilent_amd.util.normalize import normalize_tensor_positive_negative
    rng, ref = _rng(seed, "gray_cs"), reference()
    return normalize_tensor_positive_negative(_jit(rng, ref["cs_gray"]))


def gray_bank(K, seed):
    """[3,3,1,K]: 9 K values of their own, no channel a transpose or flip of another."""
    rng, ref = _rng(seed, "gray_bank%d" % K), reference()
    return _dense(rng, ref["end%d" % K])


RGB_BUILDERS = {
    "symmetric": rgb_symmetric,
    "two_group": rgb_two_group,
    "basic_blur": lambda seed: rgb_basic(seed, "blur"),
    "basic_masks": lambda seed: rgb_basic(seed, "masks"),
    "basic_dense": lambda seed: rgb_basic(seed, "dense"),
    "dense": rgb_dense,
    "nonuniform_blur": rgb_nonuniform_blur,
}
# class -> (variant, weights in the kernel's stream) of silent_rgb_chain_stream with knobs 0 (the staged path has no stream of its own)
RGB_VARIANTS = {"symmetric": (3, 149), "two_group": (2, 160), "basic_blur": (1, 265), "basic_masks": (1, 265), "basic_dense": (1, 265),
                "dense": (0, 373)}
SEED = 7            # (tests/test_chain_weights.py: the float32 evaluation keeps the most room below 1e-5 at this seed)


# what scripts/fuzz_gpu.py draws from.  tests/test_chain_weights.py runs the detection and the float32 attainability tests at each of
# them: at other seeds (0, 1, 5, 6, 8, 9 of the first ten) torch's float32 evaluation itself misses the element-wise 1e-5 rule on
# line_end for some class by up to 1.23e-5, so a failure there would say nothing about a kernel
FUZZ_SEEDS = (2, 3, 4, 7)


def rgb_weights(name, seed=SEED):
    return RGB_BUILDERS[name](seed)


# ----------------------------------------------------------------------------- index mix-ups a kernel could make

def transpose(k):
    return np.ascontiguousarray(np.asarray(k).transpose(1, 0, 2, 3))


def flip_y(k):
    return np.ascontiguousarray(np.asarray(k)[::-1])


def flip_x(k):
    return np.ascontiguousarray(np.asarray(k)[:, ::-1])


def rot180(k):
    return np.ascontiguousarray(np.asarray(k)[::-1, ::-1])


def swap_io(k):
    return np.ascontiguousarray(np.asarray(k).transpose(0, 1, 3, 2))


def channel0_profile(k):
    """A diagonal kernel with channel 0's 3 x 3 profile on every channel."""
    k = np.asarray(k)
    out = np.zeros_like(k)
    for c in range(k.shape[2]):
        out[:, :, c, c] = k[:, :, 0, 0]
    return out


MUTATIONS = {"transpose": transpose, "flip_y": flip_y, "flip_x": flip_x, "swap_io": swap_io, "channel0": channel0_profile}
# which mix-ups apply to which kernel ("blur transpose" = the folded q[d][j] read as q[j][d]; the C_in <-> C_out swap needs a
# kernel with both; the channel-0 profile is rgc's)
MUTATIONS_OF = {
    "rgc": ("transpose", "flip_y", "flip_x", "channel0"),
    "rgby": ("transpose", "flip_y", "flip_x", "swap_io"),
    "blur": ("transpose",),
    "cs_gray": ("transpose", "flip_y", "flip_x"),
}


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_chain_weights.py
# (here, because tests/test_chain_weights.py proves on the CPU that the same frames, parameters and assertions are attainable
# by a float32 evaluation and are sensitive to every mix-up above)

RGB_SHAPES = [(2, 70, 131, 3), (1, 33, 448, 3), (1, 19, 5, 3), (1, 1, 1, 3), (1, 95, 912, 3)]     # wave / tile edges of the chain kernels
PARAM_SETS = [(1.0, 0.1, 255.0, 2), (0.7, 0.25, 100.0, 1), (1.5, 0.1, 255.0, 0)]                   # (rv, root, clip_hi, pad)
GRAY_EXTENTS = [(70, 131), (35, 66), (18, 33), (9, 17), (1, 1), (32, 64), (33, 65)]


def rgb_frames(shape):
    """Noise frames; the second frame of a pair is a line drawing (black background: exact zeros, real line ends)."""
    from conftest import noise_frame, structured_frame
    n, h, w, c = shape
    frames = [noise_frame(700 + h + i, h, w, c) for i in range(n)]
    if n > 1:
        frames[1] = structured_frame(700 + h, h, w, c, 30)
    return np.stack(frames)


def dim_frames():
    """Frames on which the regulator is ACTIVE.  y = x * rv / pow(min(blur(x), 1), root): on 0 .. 255 noise the stripe responses
    reach thousands, the blurred sum is far above 1 everywhere and the 49 blur taps never reach a result; on a line drawing they
    do so only in the few pixels beside a line.  A frame of amplitude 1e-4 keeps every blurred sum below 1, and a ramp up to 1e-3
    across the width crosses 1 inside the frame (both branches of the min, and the crossing)."""
    from conftest import noise_frame
    a = noise_frame(31, 48, 70, 3) * np.float32(1e-4)
    b = noise_frame(32, 48, 70, 3) * np.linspace(0.0, 1e-3, 70, dtype=np.float32)[None, :, None]
    return np.stack([a, b.astype(np.float32)])


def dimmed(frames, k):
    """frames * 2^-k.  Scaling by a power of two is exact and everything before the regulator is positively homogeneous, so the
    stripe and blur maps of the dimmed frame are those of the frame times 2^-k, bit for bit, as long as nothing becomes denormal
    (k <= 110 on 0 .. 255 frames): every weight class and kernel form reaches any blur magnitude without new weights."""
    return (np.asarray(frames, np.float32) * np.float32(2.0 ** -int(k))).astype(np.float32)


DIM_K = (0, 13, 40, 70, 90, 100, 105, 110)      # the dimming sweep of tests/test_gpu_regulator_domain.py: blur from above 1 to 2^-113
DIM_ROOTS = (0.1, 0.5, 1.0)
DIM_RVS = (1.0, 0.7)


# ----------------------------------------------------------------------------- dyadic weights: stripe and blur exact in float32
# (tests/test_regulator_domain.py checks the premises on the CPU, tests/test_gpu_regulator_domain.py uses them: with an exact
# stripe and an exact blur the only inexact operations left in orient are the regulator's own)

EXACT_UNIT_LOG2 = {"frame": 0, "rgc": -2, "rgby": -6, "stripe": -8, "blur": -11}     # every map is an integer multiple of 2^this
DYADIC_SEED = 3


def _quarters(rng, choices, shape=None):
    return rng.choice(np.asarray(choices, np.float64), shape) / 4.0


def rgb_dyadic(seed=DYADIC_SEED):
    """Weights of the symmetric class (variant 3) whose factors are small dyadic numbers: rgc diagonal with (corner, edge_h, edge_v,
    centre) in quarters, rgby = S (x) A + B with S, A, B in quarters (S = 1 on the corners: the host's least-squares factors are then
    the quarters themselves), a channel-sum stripe in quarters, a folded channel-uniform blur in eighths (centre 1) and a two-group
    end bank of sixteenth mixes and quarter scales (scale 1 on the centre tap and on the first tap of the other group, so that
    scale * mix reconstructs every weight exactly).  On exact_frames() every partial sum of rgc, rgby, stripe and blur is an
    integer multiple of one unit (EXACT_UNIT_LOG2) below 2^24: exact in float32 in any order and any regrouping."""
    rng, ref = _rng(seed, "rgb_dyadic"), reference()
    rgc = np.zeros((3, 3, 3, 3))
    for c in range(3):
        co, eh, ev, ce = -0.25, _quarters(rng, [-1, -2]), _quarters(rng, [-1, -2]), _quarters(rng, [3, 4])
        rgc[:, :, c, c] = [[co, eh, co], [ev, ce, ev], [co, eh, co]]
    while True:
        A = _quarters(rng, [-2, -1, -1, 1], (3, 3))
        B = _quarters(rng, [-1, 1, 2], (3, 3))
        B[np.arange(3), np.arange(3)] = _quarters(rng, [3, 4], 3)
        if all(np.abs(np.cross(A[i], B[i])).max() > 0 for i in range(3)):      # A[i] not parallel to B[i]: the centre stays a group
            break
    eh, ev = rng.permutation([1, 2, 3])[:2] / 4.0
    S = np.array([[1.0, eh, 1.0], [ev, 0.0, ev], [1.0, eh, 1.0]])
    rgby = S[:, :, None, None] * A[None, None]
    rgby[1, 1] = B
    s = np.round(4.0 * _jit(rng, ref["stripe"][:, :, :1, :])) / 4.0
    s = np.where(s == 0, _quarters(rng, [-1, 1], s.shape), s)
    stripe = np.repeat(s, 3, axis=2)
    q = np.clip(np.round(8.0 * _jit(rng, ref["blur"][3:, :4, 0, 0])), 1, 8) / 8.0
    b = np.zeros((7, 7))
    for dy in range(7):
        for dx in range(7):
            b[dy, dx] = q[abs(dy - 3), min(dx, 6 - dx)]
    blur = np.repeat(np.repeat(_centre_one(b)[:, :, None, None], 3, 2), 3, 3)
    e = ref["end"].reshape(9, 3, 3)
    end = np.zeros((9, 3, 3))
    for i in range(3):
        tb = [t for t in range(9) if not END_MASKS[i] >> t & 1]
        while True:
            mix_a, mix_b = (np.round(16.0 * _jit(rng, e[t, i])) / 16.0 for t in (4, tb[0]))
            mix_a, mix_b = (np.where(m == 0, 1.0 / 16.0, m) for m in (mix_a, mix_b))
            if np.abs(np.cross(mix_a, mix_b)).max() > 0:
                break
        scale = _quarters(rng, [-3, -2, -1, 1, 2, 3], 9)
        scale[4] = 1.0
        scale[tb[0]] = 1.0          # the first and strictly largest tap of group B: the host's reference tap
        for t in range(9):
            end[t, i] = scale[t] * (mix_a if END_MASKS[i] >> t & 1 else mix_b)
    return dict(rgc=rgc, rgby=rgby, stripe=stripe, blur=blur, end=end.reshape(3, 3, 3, 3))


def exact_frames(seed=DYADIC_SEED):
    """2 x 48 x 70 x 3 frames for rgb_dyadic: 3 % (frame 0) and 6 % (frame 1) of the pixels non-zero with values 1 .. 3 per channel,
    and one black block (exact zeros: the flat policies).  Denser frames leave the 2^24 units (tests/test_regulator_domain.py)."""
    rng = _rng(seed, "exact_frames")
    frames = np.zeros((2, 48, 70, 3), np.float32)
    for f, density in enumerate((0.03, 0.06)):
        on = rng.random((48, 70)) < density
        frames[f] = np.where(on[:, :, None], rng.integers(1, 4, (48, 70, 3)), 0)
    frames[0, 8:28, 20:50] = 0.0
    return frames


EXACT_K_UNIT_AT_2M149 = 149 + EXACT_UNIT_LOG2["blur"]       # dimmed(exact_frames(), 138): the blur's unit is the smallest denormal
# where the stripe of exact_frames() is non-zero its blur spans 2^2.9 .. 2^6.7 (2^-7.4 .. where it is zero): dimmed by these k it
# lies across 1, near 2^-40 and 2^-80, across 2^-100, inside [2^-126, 2^-101], across 2^-126 and wholly in the denormals
EXACT_K = (5, 45, 85, 105, 120, 131, EXACT_K_UNIT_AT_2M149)


def regulator_allowance(y, m, root, fused):
    """|got - oracle| allowed on orient = f32(x * f32(rv / f32(pow64(m, root)))) for an EXACT stripe x and an EXACT m = min(blur, 1),
    element by element (float64).  U = 2^-24, t = root * |log2 m|.
      powf path (the per-op kernels everywhere; the fused kernels for 0 < m < 7.8886e-31 and for root == 0):  8 U |y| -- ocml's
        powf is 1 ulp = 2 U, the division and the product half an ulp each, the oracle's three roundings 1.5 U: about 4 U, doubled;
      exp2 / log2 path (the fused kernels elsewhere):  (3 ln2 t + 8) U |y| -- v_log_f32 is 1 ulp of |log2 m| (2 ln2 t U on the
        factor), the product root * log2 m half an ulp of t (ln2 t U), v_exp_f32 1 ulp, two products, the oracle's roundings.
    Plus 2^-149 for the product's rounding on either side where y is denormal (half a denormal ulp each).  Derived, not tuned;
    valid while the oracle's power stays a normal float32: the callers keep t <= 120 (root 1 may go on: pow(m, 1) = m is exact)."""
    y64, m64 = np.abs(np.asarray(y, np.float64)), np.asarray(m, np.float64)
    U = 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(m64 > 0, float(root) * np.abs(np.log2(np.where(m64 > 0, m64, 1.0))), 0.0)
    assert float(root) == 1.0 or t.max(initial=0.0) <= 120.0, "t = root * |log2 m| = %g > 120" % t.max()
    powf_path = (not fused) | (float(root) == 0.0) | ((m64 > 0) & (m64 < float(np.float32(7.8886e-31))))
    c = np.where(powf_path, 8.0, 3.0 * np.log(2.0) * t + 8.0)
    return c * U * y64 + 2.0 ** -149


BLUR_RANGES = (("m = 1", 1.0), ("2^-60 .. 1", 2.0 ** -60), ("2^-100 .. 2^-60", float(np.float32(7.8886e-31))),
               ("2^-126 .. 2^-100", 2.0 ** -126), ("denormal", 0.0))      # (name, lower edge of m = min(blur, 1))


def assert_regulator_sharp(got, want, m, root, fused, what, worst=None, form=None):
    """The sharp assertion on orient for an exact stripe and blur: where the oracle gives 0, inf or NaN the same class (zero,
    same-signed inf, NaN); elsewhere |got - want| <= regulator_allowance.  Returns the worst |err| / allowance and, with ``worst``
    (a dict), keeps the worst per (form, range of m) in it."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    m = np.broadcast_to(np.asarray(m, np.float32), want.shape)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern differs (%d vs %d)" % (what, np.isnan(got).sum(), np.isnan(want).sum())
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), "%s: infinities differ" % what
    zero = want == 0
    assert (got[zero] == 0).all(), "%s: %d of the oracle's %d zeros are not zero" % (what, (got[zero] != 0).sum(), zero.sum())
    fin = np.isfinite(want) & ~zero
    if not fin.any():
        return 0.0
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    ratio = err / regulator_allowance(want[fin], m[fin], root, fused)
    if worst is not None:
        hi = np.inf
        for name, lo in BLUR_RANGES:
            sel = (m[fin] >= lo) & (m[fin] < hi) if lo > 0 else (m[fin] < hi)
            if sel.any():
                worst[(form, name)] = max(worst.get((form, name), 0.0), float(ratio[sel].max()))
            hi = lo
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, "%s: %d / %d elements beyond the regulator's allowance; worst |err| %.3e = %.2f allowances on a value of %.6g, m = %.6g" % (
        what, (ratio > 1.0).sum(), ratio.size, err[i], ratio[i], want[fin][i], m[fin][i])
    return float(ratio[i])


def print_worst(title, worst):
    """The summary the regulator tests print (pytest -s): worst |err| / allowance per form and range of m."""
    print("\n" + title)
    for form in sorted({f for f, _ in worst}, key=str):
        print("  %-28s %s" % (form, "   ".join("%s: %.3f" % (n, worst[(form, n)]) for n, _ in BLUR_RANGES if (form, n) in worst)))


PRESCRIBED_ROOTS = (0.0, 0.1, 0.5, 1.0)


def prescribed_pixels():
    """The map of the per-op regulate test: one pixel per value, 8 columns apart (a NaN / inf pixel poisons its own 7 x 7 window only),
    the value in channel i % 3, the other two channels 0.  Returns (x, values)."""
    f = np.float32
    up, down = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    thr, two100 = f(7.8886e-31), f(2.0 ** -100)
    values = [f(-0.0), f(2.0 ** -149), down(2.0 ** -126), f(2.0 ** -126), down(thr), thr, up(thr), down(two100), two100,
              up(two100), f(2.0 ** -50), f(0.3), down(1.0), f(1.0), up(1.0), f(np.finfo(f).max), f(np.inf), f(np.nan), f(-0.5), f(-2.0)]
    x = np.zeros((1, 9, 8 * len(values) + 8, 3), f)
    for i, v in enumerate(values):
        x[0, 4, 8 * i + 8, i % 3] = v
    return x, values


def delta_blur(size, uniform):
    """A centre-delta blur: per channel (the conv kernels with the regulator epilogue) or channel-uniform (the channel-sum kernel)."""
    k = np.zeros((size, size, 3, 3))
    k[size // 2, size // 2] = 1.0 if uniform else np.eye(3)
    return k


PRESCRIBED_FORMS = (("REG conv 7x7", 7, False), ("generic conv 5x5", 5, False), ("regulate_sum", 7, True))


def check_prescribed(regulate, policy, worst):
    """``regulate(x, blur, rv, root)`` on prescribed_pixels() with the three delta blurs, every root and rv, against the oracle with the
    powf allowance (0 / inf / NaN by class)."""
    import silent_oracle as so
    x, values = prescribed_pixels()
    at = [(0, 4, 8 * i + 8, i % 3) for i in range(len(values))]
    for form, size, uniform in PRESCRIBED_FORMS:
        blur = delta_blur(size, uniform)
        with np.errstate(invalid="ignore"):
            b = so.conv2d_same(x, blur)
        m = np.where(b > 1, np.float32(1), b).astype(np.float32)
        for p, v in zip(at, values):                 # the blur IS the pixel
            assert (np.isnan(v) and np.isnan(b[p])) or b[p] == v, (form, v, b[p])
        for root in PRESCRIBED_ROOTS:
            for rv in DIM_RVS:
                with np.errstate(invalid="ignore"):
                    want = so.regulate(x, blur, rv, root, policy)
                got = regulate(x, blur, rv, root)
                assert_regulator_sharp(got, want, m, root, False, "%s root %g rv %g %s" % (form, root, rv, policy), worst, form)
        # the contract of a negative blur (include/silent_hip.h, silent_regulate), on the oracle's side: pow's own
        neg = at[len(values) - 2]                    # x = b = -0.5
        with np.errstate(invalid="ignore"):
            assert so.regulate(x, blur, 1.0, 1.0, policy)[neg] == np.float32(1.0) and so.regulate(x, blur, 0.7, 0.0, policy)[neg] == np.float32(-0.35)
            assert np.isnan(so.regulate(x, blur, 1.0, 0.5, policy)[neg]) and np.isnan(so.regulate(x, blur, 1.0, 0.1, policy)[neg])


STORE_EXTENTS = [(90, 224), (45, 112), (23, 56), (12, 28), (7, 4)]      # rows start on 16-byte boundaries (widths multiples of 4)


def store_levels():
    """The ragged pyramid of the 16-byte-store test: noise, a black block at the top of frame 0 (0 * inf under 'ieee')."""
    rng = np.random.default_rng(77)
    levels = [rng.integers(0, 256, (2, h, w, 3)).astype(np.float32) for h, w in STORE_EXTENTS]
    levels[0][0, :6, :112] = 0.0
    return levels


def staged_levels():
    """The packed levels of the staged-path test."""
    return [rgb_frames((2, 70, 131, 3)), rgb_frames((2, 35, 66, 3)), dim_frames()]


PIPELINE_HW = (150, 260)


def pipeline_frames():
    """The frames of the fused-keypoints test: noise, a line drawing, noise with a black block and a NaN and an inf pixel."""
    from conftest import noise_frame, structured_frame
    h, w = PIPELINE_HW
    frames = np.stack([noise_frame(31, h, w, 3), structured_frame(32, h, w, 3), noise_frame(33, h, w, 3)])
    frames[2, 40:60, 100:140] = 0.0
    frames[2, 70, 30, 1] = np.nan
    frames[2, 90, 200, 0] = np.inf
    return frames


def param_frames():
    from conftest import noise_frame, structured_frame
    return np.stack([noise_frame(13, 48, 70, 3), structured_frame(14, 48, 70, 3, 12)])


def gray_levels(seed, extents=GRAY_EXTENTS, n_frames=2):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (n_frames, h, w, 1)).astype(np.float32) for h, w in extents]


def assert_rgb_chain_close(got, want, bound, clip_hi, tag):
    """The end-to-end assertions on the maps of the RGB chain (``got``: orient, line_end = the padded map, value) against the
    oracle's, with the project's tolerance: 1e-5 range-relative, element-wise inside the rounding bound."""
    from conftest import assert_close
    assert_close(got["orient"], want["orient"], 1e-5, what="orient " + tag, bound=bound["orient"])
    assert_close(got["line_end"], want["padded"], 1e-5, scale=clip_hi, what="line_end " + tag, bound=bound["padded"])
    assert_close(got["value"], want["value"], 1e-5, scale=clip_hi, what="value " + tag, bound=bound["value"])


def assert_gray_chain_close(got_cs, got_end, level, want_cs, want_end, cs_kernel, bank, tag):
    import err_bound as eb
    from conftest import assert_close
    e_cs, e_end = eb.gray_chain(level, cs_kernel, bank, want_cs)
    assert_close(got_cs, want_cs, 1e-5, what="cs " + tag, bound=e_cs)
    assert_close(got_end, want_end, 1e-5, scale=255.0, what="end " + tag, bound=e_end)
