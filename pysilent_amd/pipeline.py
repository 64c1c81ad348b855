"""LineEndPipeline: the whole per-frame hot path, batched and device-resident.

Op order = the reference's graph, slam_recognition/recognition_testing.py:136-144 (callback: frame ->
zoom pyramid) and :69-90 (compile: rgc -> rgby -> orientation -> line-end -> clip -> pad -> value ->
keypoint indices), restated for the two workloads of BASELINE.json:

  mode "gray"  (configs 1, 2, 5)  frame[H,W,1] -> pyramid -> CS -> ReLU -> K-orientation end bank -> ReLU -> clip
  mode "rgb"   (config 3)         frame[H,W,3] -> pyramid -> rgc -> rgby -> stripe -> regulate -> end -> clip
                                   -> pad_inwards -> value -> per-region keypoint indices

All buffers are torch GPU tensors allocated once; every launch goes to torch's current stream through the
``*_dev`` C-ABI entry points, so a step is pure kernel launches (no allocation, no synchronisation).
PyTorch is used for device memory and streams only.
"""
import ctypes as C
import fractions

import numpy as np

from . import _lib, _runtime
from . import constant_convolutions as cc
from .util.normalize import normalize_tensor_positive_negative
from .util.zoom.from_image import classic_levels, reference_levels


def default_constants(mode, n_orient=4):
    """The constant kernels of a pipeline as one dict of float32 HWIO arrays (what gets broadcast)."""
    if mode == "gray":
        cs = normalize_tensor_positive_negative(cc.center_surround_tensor(2, [1], [1], [1], [-1]))
        return {"cs": cs.astype(np.float32), "end": cc.end_bank(n_orient).astype(np.float32)}
    if mode == "rgb":
        return {"rgc": cc.midget_rgc(2).astype(np.float32), "rgby": cc.rgby_3(2).astype(np.float32),
                "stripe": cc.rgb_2d_stripe_tensors().astype(np.float32), "blur": cc.blur_tensor(2, 7).astype(np.float32),
                "end": cc.rgb_2d_end_tensors().astype(np.float32)}
    raise ValueError("mode must be 'gray' or 'rgb'")


def pack_constants(consts):
    """dict of arrays -> (flat float32 blob, layout) for a single broadcast."""
    layout, parts = [], []
    for name in sorted(consts):
        a = np.ascontiguousarray(consts[name], dtype=np.float32)
        layout.append((name, a.shape))
        parts.append(a.reshape(-1))
    return np.concatenate(parts), layout


def unpack_constants(blob, layout):
    out, off = {}, 0
    for name, shape in layout:
        n = int(np.prod(shape))
        out[name] = np.asarray(blob[off:off + n], dtype=np.float32).reshape(shape).copy()
        off += n
    return out


def _spin_ms(torch, dev, streams, microseconds):
    """Wall time of one busy-wait kernel (silent_busy_wait_dev: one wavefront polling the clock) on each of ``streams`` at once."""
    import time
    ctx = _runtime.get_context(dev.index)
    lib = _lib.load()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for st in streams:
        ctx.check(lib.silent_busy_wait_dev(ctx.handle, int(microseconds), C.c_void_p(st.cuda_stream)))
    for st in streams:
        st.synchronize()
    return (time.perf_counter() - t0) * 1e3


def pick_concurrent_stream(torch, dev, beside, priority=0, tries=10, microseconds=400):
    """A new stream whose work really runs CONCURRENTLY with the streams in ``beside``.  HIP multiplexes streams onto a few
    hardware queues, and two streams that share one are served strictly in order -- "overlap" through such a pair is a loss
    (cross-stream events, no concurrency), and which pairs share is a property of the process's stream pool, not of the
    priorities (scripts/ab_overlap_pool.py: pipelines #2, #5 and #7 of a process lost 40 %, the others won 8 %).  So it is
    measured: a spin kernel on the candidate and on every stream of ``beside`` at once must take about as long as one alone
    (about a millisecond each).  A NECESSARY check only: pairs that pass it can still stall each other through the real step's
    cross-stream events -- tune_overlap times the real thing.  Returns (stream, verified); after ``tries`` candidates the last one
    is returned unverified (callers keep the flag: LineEndPipeline.overlap_verified)."""
    one = min(_spin_ms(torch, dev, beside[:1] or [torch.cuda.current_stream(dev)], microseconds) for _ in range(2))
    cand = None
    keep = []                                  # rejected candidates stay alive until the choice is made (the pool hands out new ones)
    for _ in range(tries):
        cand = torch.cuda.Stream(dev, priority=priority)
        together = min(_spin_ms(torch, dev, list(beside) + [cand], microseconds) for _ in range(2))
        if together < 1.5 * one:
            return cand, True
        keep.append(cand)
    return cand, False


_staging_pool = None


def _staging_copy(dst, src, min_bytes=8 << 20, workers=16):
    """Pageable host frames -> the pinned staging buffer.  One memcpy thread moves ~5 GB/s, a tenth of what the link then takes
    away: batches above ``min_bytes`` are split along the batch axis over a small thread pool (NumPy releases the GIL in copyto)."""
    global _staging_pool
    nbytes = src.numel() * src.element_size()
    n = min(workers, int(src.shape[0]))
    if nbytes < min_bytes or n < 2:
        dst.copy_(src)
        return
    if _staging_pool is None:
        from concurrent.futures import ThreadPoolExecutor
        _staging_pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="silent-staging")
    d, s_ = dst.numpy(), src.numpy()
    step = -(-int(src.shape[0]) // n)
    list(_staging_pool.map(lambda i: np.copyto(d[i:i + step], s_[i:i + step]), range(0, int(src.shape[0]), step)))


class _RawBlock(object):
    """A device allocation of the library's own (silent_malloc / silent_free): the placement tuner's spacers and draws."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        ctx.check(_lib.load().silent_malloc(ctx.handle, C.c_size_t(self.nbytes), C.byref(p)))
        self.ptr = int(p.value)

    def __del__(self):
        try:
            if getattr(self, "ptr", 0):
                _lib.load().silent_free(self.ctx.handle, C.c_void_p(self.ptr))
                self.ptr = 0
        except Exception:
            pass


# The keywords of the attention tail (LineEndPipeline(..., mode="rgb", attention=True, centroid_region=(3, 3), ...)) and their defaults
ATTENTION_KEYWORDS = dict(attention=False, centroid_region=(3, 3), input_based_recovery=False, constant_recovery=True, attention_visualize=True)


# rgb_storage="float16" (mode "rgb"): the orient and line_end maps are stored as float16 (silent_rgb_line_end_h / silent_rgb_keypoints_h).
# A keyword of its own: storage="float16" keeps raising on mode "rgb" (pinned by the suite), and it travels like the attention keywords
RGB_STORAGE_KEYWORDS = dict(rgb_storage="float32")


class _PipelineCall(type):
    """The call ``LineEndPipeline(...)``: the keywords of ATTENTION_KEYWORDS and RGB_STORAGE_KEYWORDS are taken off the arguments and
    handed to the instance before ``__init__`` runs, which reads them where it checks its other arguments.  ``__init__`` keeps its
    parameter list: that list is pinned by the suite (the source keywords are its last four), and these belong to optional stages /
    forms of the step."""

    def __call__(cls, *args, **kw):
        self = cls.__new__(cls)
        self._attention_keywords = dict(ATTENTION_KEYWORDS, **{k: kw.pop(k) for k in ATTENTION_KEYWORDS if k in kw})
        self._rgb_storage_keywords = dict(RGB_STORAGE_KEYWORDS, **{k: kw.pop(k) for k in RGB_STORAGE_KEYWORDS if k in kw})
        self.__init__(*args, **kw)
        return self


class LineEndPipeline(object, metaclass=_PipelineCall):
    rgb_storage = "float32"      # (the default of RGB_STORAGE_KEYWORDS: what an instance that never ran __init__ reports)

    def __init__(self, frame_hw, mode="gray", n_levels=5, scale=2.0, n_orient=4, batch=1, device=None,
                 constants=None, center_dimensions=None, clip_hi=255.0, flat_policy="ieee", pad=2,
                 max_keypoints_per_frame=None, selection=False, top_percent=0.1, keep_selection_maps=False, value_map=None,
                 peak_value_map=None, orient_map=True, overlap=False, overlap_priorities=True, placement="auto", keypoints=False,
                 regions=None, accumulation="float32", storage="float32", frame_dtype="float32", frame_channels=1,
                 frame_layout="packed", rgb_frame_dtype="float32", rgb_frame_layout="packed", rgb_frame_format="interleaved",
                 nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr"):
        # rgb_frame_dtype="uint8" (mode "rgb"): step() takes packed interleaved uint8 colour frames [batch, H, W, 3] as a camera or a
        # decoder delivers them and the pyramid kernels read the bytes themselves (silent_pyramid_rgb8_dev) -- no widening cast, no
        # float32 copy of the batch; the pyramid, and with it every map and keypoint, is bit-identical to the float32 pipeline's on
        # the widened frames.  A keyword of its own: frame_dtype / frame_channels / frame_layout describe the frames of mode "gray" and
        # keep their refusals on mode "rgb".  Checked first, before any GPU or torch work: unknown names, mode "gray", and "uint8"
        # beside a non-default frame_dtype / frame_channels / frame_layout
        self.rgb_frame_dtype = _runtime.check_rgb_frame_dtype(rgb_frame_dtype, mode, frame_dtype, frame_channels, frame_layout)
        # rgb_frame_layout="strided" (mode "rgb", rgb_frame_dtype="uint8"): step() takes ANY uint8 GPU view [batch, H, W, 3] with
        # positive strides and channel stride 1 -- bgra[..., :3], a pitched BGR surface, a region of larger frames -- and the pyramid
        # kernels read it in place (silent_pyramid_rgb8_view_dev): no packing launch, no second copy of the batch; pyramid, maps and
        # keypoints are those of the packed uint8 pipeline on view.contiguous(), bit for bit.  step_host is unchanged (its staging
        # copy packs).  A keyword of its own like rgb_frame_dtype; refused here: unknown names, mode "gray", rgb_frame_dtype="float32",
        # a non-default frame_dtype / frame_channels / frame_layout
        self.rgb_frame_layout = _runtime.check_rgb_frame_layout(rgb_frame_layout, mode, rgb_frame_dtype, frame_dtype, frame_channels,
                                                                frame_layout)
        # rgb_frame_format="nv12" (mode "rgb"): step() takes a pair (y, uv) of uint8 GPU planes as a hardware video decoder emits
        # them -- luma [batch, H, W], interleaved chroma [batch, H / 2, W / 2, 2], both pitched (util.zoom.nv12_planes cuts them out
        # of surface tensors) -- and the pyramid kernels read them in place, converting (Y, U, V) to three float32 channels in
        # registers (silent_pyramid_nv12_dev): no conversion launch, no 12 B/px copy of the batch; pyramid, maps and keypoints are
        # those of the float32 pipeline on _runtime.nv12_to_rgb(planes), bit for bit.  nv12_matrix ("bt601" / "bt709" or a 3 x 3
        # array), nv12_range ("limited" / "full") and nv12_order ("bgr" / "rgb") choose the coefficients (_runtime.nv12_coefficients).
        # Refused here, before any GPU or torch work: unknown names, mode "gray", rgb_frame_dtype="uint8", rgb_frame_layout="strided",
        # non-default frame_dtype / frame_channels / frame_layout, odd H or W
        self.rgb_frame_format = _runtime.check_rgb_frame_format(rgb_frame_format, mode, rgb_frame_dtype, rgb_frame_layout, frame_dtype,
                                                                frame_channels, frame_layout, frame_hw)
        # rgb_frame_format="p010" / "p012" / "p016": the same pair as uint16 planes, as the decoders emit them for 10- and 12-bit
        # streams -- the code value in the high 10 / 12 / 16 bits of each element (util.zoom.p010_planes) -- read in place by
        # silent_pyramid_p010_dev; the converted channels are on the 0 .. 255 scale and NOT rounded, so the extra bits of a 10-bit source
        # reach the pyramid; pyramid, maps and keypoints are those of the float32 pipeline on _runtime.p010_to_rgb(planes, depth=...),
        # bit for bit.  The nv12_* keywords describe the conversion for these formats too (_runtime.p010_coefficients), and
        # nv12_matrix="bt2020" exists for them only.
        # rgb_frame_format="yuv420" / "yuv422" / "yuv444": the frames are a TRIPLE (y, u, v) of uint8 GPU views of any positive strides
        # -- planar I420 / YV12 / I422 / I444 as software and JPEG decoders emit them, semi-planar NV21 / NV16, packed YUYV / UYVY of a
        # UVC webcam (yuyv[:, :, 0::2], yuyv[:, :, 1::4], yuyv[:, :, 3::4]); util.zoom.yuv_planes cuts them out of surfaces -- read in
        # place by silent_pyramid_yuv_dev, one byte per load; pyramid, maps and keypoints are those of the float32 pipeline on
        # _runtime.yuv_to_rgb(planes, fmt=...), bit for bit.  The nv12_* keywords describe the conversion, as for "nv12".
        # rgb_frame_format one of _runtime.YUV16_FORMATS ("yuv420p10", "yuv422p10msb", "yuv444p16" ...): the same triple as UINT16 GPU
        # views -- yuv420p10le / I010 planes of a software decoder (the code in the low bits), P210 / P410 surfaces and packed Y210 (the
        # code in the high bits: "...msb"); util.zoom.yuv16_planes cuts them out of surfaces -- read in place by
        # silent_pyramid_yuv16_dev, one element per load; pyramid, maps and keypoints are those of the float32 pipeline on
        # _runtime.yuv16_to_rgb(planes, fmt=...), bit for bit.  The conversion is P010's (_runtime.p010_coefficients at the format's
        # depth; "bt2020" is accepted).
        # rgb_frame_format="bayer_rggb" / "bayer_grbg" / "bayer_gbrg" / "bayer_bggr" (util.zoom.BAYER_LAYOUTS maps the GenICam names): the
        # frames are ONE uint8 GPU view [batch, H, W] (or [batch, H, W, 1]) of a raw Bayer mosaic as a machine-vision camera delivers
        # it, any positive strides, the name that of the top-left 2 x 2 cell of the view -- read in place by silent_pyramid_bayer_dev and
        # demosaiced (bilinear) in registers, 1 B/px; pyramid, maps and keypoints are those of the float32 pipeline on
        # _runtime.bayer_to_rgb(frames, hw, fmt), bit for bit.  nv12_order selects "bgr" / "rgb" as for every other source; a non-default
        # nv12_matrix or nv12_range is refused (they would silently mean nothing).  H and W of at least 2, odd extents allowed.
        if self._bayer is not None:
            _runtime.check_bayer_conversion(self.rgb_frame_format, nv12_matrix, nv12_range, nv12_order)   # (for its refusals)
            self.nv12_order = nv12_order
        if self._source and self._source[0].elem == 2:
            self.nv12_m, self.nv12_oy, self.nv12_oc = _runtime.p010_coefficients(nv12_matrix, nv12_range, nv12_order, self._source[3])
        else:
            self.nv12_m, self.nv12_oy = _runtime.nv12_coefficients(nv12_matrix, nv12_range, nv12_order)
        # accumulation="float64" (mode "gray"): every op sums its taps in float64 and rounds once to float32, like the CPU oracle
        # (SILENT_PLAN_ACCUM_F64: the pyramid within 1 ulp of it, CS and end bit-identical to it on the same pyramid).  Checked first:
        # no GPU or torch work for a refused argument
        _runtime.check_accumulation(accumulation)
        if accumulation == "float64" and mode != "gray":
            raise ValueError("accumulation='float64' is for mode 'gray' (the RGB chain accumulates in float32)")
        self.accumulation = accumulation
        # storage="float16" (mode "gray"): the CS and end maps are stored as float16 (silent_gray_pass_h_dev) -- every element the
        # float32 result rounded to nearest even, half the bytes written and kept; the pyramid stays float32.  Also refused before
        # any GPU or torch work: unknown names, mode "rgb", accumulation="float64", keypoints=True
        self.storage = _runtime.check_storage(storage, mode, accumulation, bool(keypoints))
        # rgb_storage="float16" (mode "rgb"): orient and line_end are stored as float16 (silent_rgb_line_end_h_dev /
        # silent_rgb_keypoints_h_dev) -- every element the float32 result rounded once at the store, half the bytes written and
        # kept for the pipeline's two largest maps; pyramid, value, peak_value and the attention tail stay float32.  Without
        # selection the keypoints are the float32 pipeline's bit for bit (they come from the value map); with selection they are
        # silent_rgb_keypoints_h's (include/silent_hip.h: ties).  Refused before any GPU or torch work: unknown names, mode "gray",
        # keep_selection_maps=True
        self.rgb_storage = _runtime.check_rgb_storage(getattr(self, "_rgb_storage_keywords", RGB_STORAGE_KEYWORDS)["rgb_storage"], mode,
                                                      bool(keep_selection_maps))
        # frame_dtype="uint8" (mode "gray"): step() takes uint8 frames as a camera or decoder delivers them and the kernels read the
        # bytes themselves (the silent_*_u8 entry points) -- no widening cast, no float32 copy of the batch, every map bit-identical
        # to the float32 pipeline's on the widened frames.  Refused here as well: unknown names, mode "rgb", accumulation="float64"
        # (checked below, after frame_channels: a refused frame_channels=3 is reported as such)
        # frame_dtype="uint16" (mode "gray"): the same for unsigned 16-bit frames in native byte order (the silent_*_u16 entry points:
        # Mono10 / 12 / 16, Y16 / Z16, the luma of P010 / P016) -- the value is (float)v, exact, no shift and no scale: a P010 source
        # (10 bits in the HIGH bits) passes clip_hi * 64 and reads maps exactly 64 times the 10-bit ones.  Refused here as well: mode
        # "rgb", accumulation="float64", frame_channels=3
        # frame_channels=3 (mode "gray", frame_dtype="uint8"): step() takes [batch, H, W, 3] interleaved colour uint8 frames and the
        # kernels form each pixel's value (b0 + b1 + b2) * float32(1/3) at the load (the silent_*_u8x3 entry points) -- no cast launch,
        # no value launch, no float32 buffer; every map bit-identical to the float32 pipeline's on the frame of values.  frame_shape
        # becomes (H, W, 3); channels, the plan and all maps stay single-channel.  Refused here as well: anything but 1 and 3, and 3
        # with mode "rgb", frame_dtype="float32" or "uint16", or accumulation="float64"
        self.frame_channels = _runtime.check_frame_channels(frame_channels, mode, frame_dtype, accumulation)
        self.frame_dtype = _runtime.check_frame_dtype(frame_dtype, mode, accumulation)
        # frame_layout="strided" (mode "gray", frame_dtype="uint8"): step() takes ANY uint8 GPU view of the right shape with positive
        # strides -- surface[:, :H, :W, None] of a pitched NV12 batch, bgra[..., :3], yuyv[:, :, ::2, None], a region of larger frames
        # -- and the kernels read it in place (the silent_*_view entry points): no packing launch, no second copy of the batch, every
        # map bit-identical to the packed pipeline's on the compacted pixels.  step_host is unchanged (its staging copy packs).
        # With frame_dtype="uint16" any uint16 GPU view (the silent_*_view16 entry points: p010[:, :H, :W] of pitched surfaces,
        # rgba16[..., 1], a window of larger frames).
        # Refused here as well: unknown names, mode "rgb", frame_dtype="float32", accumulation="float64"
        self.frame_layout = _runtime.check_frame_layout(frame_layout, mode, frame_dtype, accumulation)
        # attention=True (mode "rgb"): after the chain every step runs the second half of the reference's graph
        # (recognition_testing.py:77-100) on the step's value map -- centroid maps at two scales and get_boosting with a per-stream
        # energy state -- in two launches (silent_attention_tail_dev): every frame slot of the batch is a camera stream of its own,
        # ``energy`` its state.  centroid_region, input_based_recovery / constant_recovery and attention_visualize are the reference's
        # centroid_region_shape[1:3], its two recovery flags and get_boosting's for_visualizing.  Refused here, before any GPU or torch
        # work: mode "gray", value_map=False, overlap, a region extent below 1, no recovery, a level too small for a half extent
        attention, centroid_region, input_based_recovery, constant_recovery, attention_visualize = (
            getattr(self, "_attention_keywords", ATTENTION_KEYWORDS)[k] for k in ATTENTION_KEYWORDS)
        self.attention = bool(attention)
        if self.attention:
            if mode != "rgb":
                raise ValueError("attention=True is for mode 'rgb' (the tail reads the RGB chain's value map)")
            if value_map is not None and not value_map:
                raise ValueError("attention=True needs the value map: value_map=False is refused")
            if overlap not in (False, None):
                raise ValueError("attention=True does not support overlap (overlapped steps with the tail are not built)")
            self._attention_params = self._checked_attention_params(frame_hw, center_dimensions, scale, n_levels, centroid_region,
                                                                    input_based_recovery, constant_recovery, attention_visualize)
        if self.rgb_frame_dtype == "uint8":
            self.frame_dtype = "uint8"         # what step() takes: the ingest ring, the tuners' frames and the byte accounting follow it
        import torch
        self.torch = torch
        self.mode = mode
        self.channels = 1 if mode == "gray" else 3
        self.device_index = _runtime.default_device() if device is None else int(device)
        self.tdev = torch.device("cuda", self.device_index)
        self.ctx = _runtime.get_context(self.device_index)
        self.batch = int(batch)
        h, w = int(frame_hw[0]), int(frame_hw[1])
        self.frame_shape = (h, w, 3 if self.frame_channels == 3 else self.channels)
        levels = (reference_levels((h, w), center_dimensions, scale) if center_dimensions is not None
                  else classic_levels((h, w), scale, n_levels))
        self.crop_px = None
        if center_dimensions is not None:
            y0 = min(l[0] for l in levels); x0 = min(l[1] for l in levels)
            y1 = max(l[0] + l[2] for l in levels); x1 = max(l[1] + l[3] for l in levels)
            self.crop_px = (y1 - y0) * (x1 - x0)
        self.plan = _runtime.PyramidPlan(h, w, self.channels, levels, self.device_index, accumulation=accumulation)
        self.extents = self.plan.extents
        self.frame_px = self.plan.frame_px
        self.n_levels = len(self.extents)
        self.levels_c = (_lib.Extent * self.n_levels)(*[_lib.Extent(eh, ew) for eh, ew in self.extents])
        self.consts = {k: np.ascontiguousarray(v, np.float32) for k, v in
                       (constants or default_constants(mode, n_orient)).items()}
        self.clip_hi, self.flat_policy, self.pad = float(clip_hi), flat_policy, int(pad)
        n = self.batch * self.frame_px
        f32 = dict(dtype=torch.float32, device=self.tdev)
        self.placement_tuning = None
        # overlap: consecutive steps overlap on two internal streams -- rgb: the pyramid of batch n + 1 (latency-bound walk kernel)
        # beside the chain kernel and the small launches of the keypoint tail of batch n; gray: the single-read stream kernel of
        # batch n + 1 beside the filter kernel of batch n's smaller levels.  The pyramid is then double-buffered (pipeline.pyr = the
        # last step's).  step() stays "enqueue the whole path for this batch", but on the
        # pipeline's own streams: wait() orders the caller's stream behind the results, outputs() does so itself.
        # overlap=True and overlap="auto" both MEASURE (tune_overlap): a pair of streams that does not pay -- some pairs of a
        # process's stream pool lose 30 - 40 % -- is never kept on faith.  overlap="force": the first pair, unmeasured (tests of
        # the overlapped path's bit-identity, A/B scripts)
        if overlap not in (False, True, None, "auto", "force"):
            raise ValueError("overlap must be False, True, 'auto' or 'force'")
        self._overlap_auto = overlap in (True, "auto")
        self._chain_priority = -1 if overlap_priorities else 0
        self.overlap = False
        self.overlap_verified = None
        self.overlap_tuning = None
        self._order_caller = True          # (A/B switch of scripts/ab_overlap.py: order the caller's stream behind the frame read)
        self._chain_stream = self._walk_stream = self._copy_stream = None
        # keypoints (gray only; rgb always computes them): the gray pass with its keypoint epilogue and the selection tail in one
        # C-ABI call (silent_gray_keypoints_dev).  value_map / peak_value_map: keep those maps (gray default: no, rgb default: yes)
        self.keypoints = mode != "gray" or bool(keypoints)
        if mode == "gray":
            self.n_orient = int(self.consts["end"].shape[3])
            if keypoints:
                if overlap not in (False, None):
                    raise ValueError("keypoints=True does not support overlap (the two-part gray step)")
                if keep_selection_maps:
                    raise ValueError("keep_selection_maps is for mode 'rgb'; gray keypoints keep value / peak_value maps only")
                self.selection, self.top_percent = bool(selection), float(top_percent)
                self.value = torch.empty(n, **f32) if value_map else None
                self.peak_value = torch.empty(n, **f32) if (peak_value_map and self.selection) else None
                if peak_value_map and not self.selection:
                    raise ValueError("peak_value_map needs selection=True")
            elif regions is not None:
                raise ValueError("regions need keypoints=True in mode 'gray'")
        else:
            value_map = True if value_map is None else value_map
            peak_value_map = True if peak_value_map is None else peak_value_map
            # orient_map=False: SURVEY.md section 8d config 3 returns line_end + keypoints, the orientation map is optional
            self.orient_map = bool(orient_map)
            # value_map=False: the value map (a-8 of the line-end map) is not kept -- with selection the fused step needs it
            # nowhere (silent_rgb_keypoints), and BASELINE config 3 returns line_end + keypoints (+ orient) only
            self.value_map = bool(value_map) or not selection or bool(keep_selection_maps)
        self._adopt_maps(self._alloc_maps())
        if self.attention:
            self._alloc_attention()
        if self.keypoints:
            # regions: one (rH, rW) per level (default: half the level) -- the strides of max_value_indices_region's pool, TF1
            # max_pool(k = the whole level, stride = region, SAME): a pixel is a keypoint where it reaches the maximum of its window.
            # More than 4 windows per axis on any level runs the general window-maxima path for the whole call, without the sparse tail
            if regions is None:
                regions = [(max(eh // 2, 1), max(ew // 2, 1)) for eh, ew in self.extents]
            if len(regions) != self.n_levels:
                raise ValueError("need one (rH, rW) region per level (%d levels, %d regions)" % (self.n_levels, len(regions)))
            self.regions = (_lib.Extent * self.n_levels)(*[_lib.Extent(int(rh), int(rw)) for rh, rw in regions])
            self.kp_cap = int(max_keypoints_per_frame or self.frame_px)
            self.kp_idx = torch.empty((self.batch, self.kp_cap, 4), dtype=torch.int64, device=self.tdev)
            self.kp_counts = torch.zeros(self.batch, dtype=torch.int64, device=self.tdev)
        if mode != "gray":
            # selection=True: SURVEY.md section 8d config 3 -- top-percent threshold (a-10, p = 0.1), 3x3 NMS (a-9),
            # then the per-region keypoint indices (a-11) of what survives; False: the reference graph
            # (recognition_testing.py:90), keypoints straight from the padded line-end map
            self.selection, self.top_percent = bool(selection), float(top_percent)
            self.keep_selection_maps = bool(keep_selection_maps)
            if self.selection:
                if self.keep_selection_maps:
                    self.top = torch.empty(n * 3, **f32)
                    self.peaks = torch.empty(n * 3, **f32)
                # peak_value_map=False (fused step only): nobody wants the selection's value map itself -- the keypoint tail
                # then runs sparse (silent_rgb_keypoints with peak_value_out = NULL, csrc/silent_peaks.h)
                self.peak_value_map = bool(peak_value_map) or self.keep_selection_maps
                self.peak_value = torch.empty(n, **f32) if self.peak_value_map else None
            fp = C.POINTER(C.c_float)
            self._params = _lib.RgbChainParams(
                *[self.consts[k].ctypes.data_as(fp) for k in ("rgc", "rgby", "stripe", "blur", "end")],
                1.0, 0.1, {"ieee": _lib.FLAT_IEEE, "zero": _lib.FLAT_ZERO}[flat_policy], self.clip_hi, self.pad)
        self._lib = _lib.load()
        # placement="auto" (default): the first batch ``step`` sees tunes the placement of the small maps against the big one AND
        # against that batch's own buffer (tune_placement: <= 1 s, bounded memory, results unaffected); None / False: the maps
        # stay where the constructor's allocations landed -- side by side, which is the slow relation more often than not
        if placement not in (None, False, "auto"):
            raise ValueError("placement must be None or 'auto'")
        self._placement_pending = placement == "auto"
        if overlap == "force":
            self._pyrs.append(torch.empty_like(self._pyrs[0]))
            # the chain + tail of batch n are the critical path, the pyramid of batch n + 1 only has to be ready in time: the chain's
            # stream gets the higher queue priority, the pyramid's stream is checked to run concurrently with it
            self._new_stream_pair()
            self.overlap = True
        elif self._overlap_auto:
            self.tune_overlap()

    # -- attention=True: the tail's geometry, state and outputs ---------------------------------------------
    @staticmethod
    def _checked_attention_params(frame_hw, center_dimensions, scale, n_levels, centroid_region, input_based_recovery, constant_recovery,
                                  visualize):
        """The silent_attention_params of the constructor's keywords, checked against the pyramid's level extents (host work only:
        the level generators and silent_attention_extents).  Every refusal names ``attention``."""
        from .util.energy.recovery import recovery_mode
        try:
            rh, rw = (int(v) for v in centroid_region)
        except (TypeError, ValueError):
            raise ValueError("attention=True: centroid_region must be a pair (rH, rW)")
        if rh < 1 or rw < 1:
            raise ValueError("attention=True: the extents of centroid_region must be >= 1, got %s" % ((rh, rw),))
        try:
            mode = recovery_mode(input_based_recovery, constant_recovery)
        except ValueError as e:
            raise ValueError("attention=True: %s" % e)
        params = _runtime.attention_params((rh, rw), recovery_mode=mode, visualize=visualize)
        hw = (int(frame_hw[0]), int(frame_hw[1]))
        levels = reference_levels(hw, center_dimensions, scale) if center_dimensions is not None else classic_levels(hw, scale, n_levels)
        try:
            _runtime.attention_extents([(l[6], l[7]) for l in levels], params)
        except ValueError as e:
            raise ValueError("attention=True: %s" % e)
        return params

    def _alloc_attention(self):
        """The state (8 in every cell: boosting.py:6-7) and the four results of the tail, allocated ONCE: they are no part of a
        placement draw (tune_placement)."""
        torch = self.torch
        self.attention_cells, self.attention_half, self.attention_cells2 = _runtime.attention_extents(self.extents, self._attention_params)
        self.attention_channels = 3 if self._attention_params.boosting.visualize else 1
        self.cells_per_frame = sum(h * w for h, w in self.attention_cells)
        f32 = dict(dtype=torch.float32, device=self.tdev)
        self.energy = torch.full((self.batch, self.cells_per_frame), 8.0, **f32)
        self.centroids = torch.empty(self.batch * self.frame_px, **f32)
        self.centroids2 = torch.empty(self.batch * sum(h * w for h, w in self.attention_half), **f32)
        self.fired = torch.empty(self.batch * self.cells_per_frame * self.attention_channels, **f32)
        self.update = torch.empty(self.batch * self.cells_per_frame * self.attention_channels, **f32)
        self._attention_state = self.energy          # what run_attention advances: a scratch copy while a tuner times steps

    def run_attention(self, stream=None):
        """The tail on the step's value map (silent_attention_tail_dev): advances every slot's state by one step."""
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self._lib.silent_attention_tail_dev(
            self.ctx.handle, p(self.value), self.levels_c, self.n_levels, self.batch, C.byref(self._attention_params),
            p(self._attention_state), p(self.centroids), p(self.centroids2), p(self.fired), p(self.update), stream or self._stream()))

    def _parked_state(self):
        """Context of a tuner's timed steps: they run the tail on a SCRATCH state, so no stream advances (bit for bit)."""
        import contextlib

        @contextlib.contextmanager
        def parked():
            if not self.attention:
                yield
                return
            self._attention_state = self.energy.clone()
            try:
                yield
            finally:
                self.torch.cuda.synchronize(self.tdev)
                self._attention_state = self.energy
        return parked()

    def get_state(self):
        """Host copy of the boosting state, [batch, cells per frame] (attention=True)."""
        self._need_attention("get_state")
        return self.energy.cpu().numpy()

    def set_state(self, state):
        self._need_attention("set_state")
        state = np.ascontiguousarray(state, np.float32)
        if tuple(state.shape) != tuple(self.energy.shape):
            raise ValueError("state shape %s does not match [batch, cells per frame] = %s" % (state.shape, tuple(self.energy.shape)))
        self.energy.copy_(self.torch.from_numpy(state))

    def reset_state(self, slots=None):
        """8 in every cell of the named frame slots (default: all) -- a camera that reconnects starts a new stream."""
        self._need_attention("reset_state")
        if slots is None:
            self.energy.fill_(8.0)
            return
        for s in slots:
            if not 0 <= int(s) < self.batch:
                raise ValueError("reset_state: slot %d of a batch of %d" % (int(s), self.batch))
            self.energy[int(s)].fill_(8.0)

    def _need_attention(self, what):
        if not self.attention:
            raise ValueError("%s needs attention=True" % what)

    # -- the maps a step streams through: pyramid + every dense output ---------------------------------
    def _alloc_maps(self):
        """Fresh device buffers for the pyramid and the dense maps (one allocation each; the keypoint rows and the optional
        selection maps are not part of it)."""
        torch = self.torch
        n = self.batch * self.frame_px
        f32 = dict(dtype=torch.float32, device=self.tdev)
        m = {"pyr": torch.empty(n * self.channels, **f32)}
        if self.mode == "gray":
            maps = dict(f32, dtype=torch.float16) if self.storage == "float16" else f32
            m["cs"] = torch.empty(n, **maps)
            m["end"] = torch.empty(n * self.n_orient, **maps)
        else:
            maps = dict(f32, dtype=torch.float16) if self.rgb_storage == "float16" else f32
            m["orient"] = torch.empty(n * 3, **maps) if self.orient_map else None
            m["line_end"] = torch.empty(n * 3, **maps)
            m["value"] = torch.empty(n, **f32) if self.value_map else None
        return m

    def _adopt_maps(self, m):
        """Make ``m``'s tensors the pipeline's maps ("pyr1": the second pyramid buffer of an overlapped pipeline).  Views an earlier
        ``outputs()`` handed out keep the OLD tensors (alive, no longer written): call ``outputs()`` again after a tuner ran."""
        self._pyrs = [m["pyr"]] + ([m["pyr1"]] if "pyr1" in m else list(getattr(self, "_pyrs", [])[1:]))
        self.pyr = self._pyrs[0]
        for k, v in m.items():
            if k not in ("pyr", "pyr1"):
                setattr(self, k, v)

    def _synthetic_frames(self):
        """Noise frames of the dtype step() takes (the tuners' default batch)."""
        torch = self.torch
        if self._source:
            src, _, _, depth, shift = self._source
            return tuple((torch.randint(0, 1 << depth, sh, device=self.tdev) << shift).to(getattr(torch, src.dtype)) for sh in self._plane_shapes())
        if self._bayer is not None:
            return torch.randint(0, 256, (self.batch,) + self.frame_shape[:2], device=self.tdev).to(torch.uint8)
        frames = torch.randint(0, 256, (self.batch,) + self.frame_shape, device=self.tdev)
        return frames.to(self._frame_torch_dtype)

    def _time_step(self, frames, steps, windows=2):
        import time
        torch = self.torch
        best = None
        for _ in range(windows):
            torch.cuda.synchronize(self.tdev)
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step(frames)
            torch.cuda.synchronize(self.tdev)
            t = (time.perf_counter() - t0) / steps * 1e3
            best = t if best is None else min(best, t)
        return best

    def _raw_tensor(self, like):
        """A device buffer of ``like``'s shape and dtype from the library's allocator (silent_malloc: a plain hipMalloc, given back
        to the driver by silent_free the moment the last reference goes), wrapped as a torch tensor.  The tuner's draws and
        spacers come from here, not from torch's caching allocator: nothing a draw leaves behind stays cached in the process."""
        nbytes = like.numel() * like.element_size()
        owner = _RawBlock(self.ctx, nbytes)
        typestr = {4: "<f4", 1: "|u1", 8: "<i8", 2: "<f2"}[like.element_size()]
        owner.__cuda_array_interface__ = {"shape": tuple(like.shape), "typestr": typestr, "data": (owner.ptr, False), "version": 2}
        t = self.torch.as_tensor(owner, device=self.tdev)      # (holds a reference to ``owner`` for as long as the tensor lives)
        assert t.data_ptr() == owner.ptr
        return t

    def tune_placement(self, frames=None, tries=10, steps=8, budget_s=1.0, spacer_gib=None, max_held_gib=None):
        """Pick the physical placement of the maps RELATIVE to each other by measurement; the largest map is moved last.

        What is measured (profiles/r06/placement.md): the step's time depends on where the maps lie relative to each other in the
        device's physical memory -- not on where any one of them lies.  The same K-orientation map is fast with one allocation of
        the CS map + pyramid and 25 % slower with another (1.18 vs 1.52 ms for config 5's dominant kernel), and the other way
        round for another K map; a synthetic kernel that only issues the three store streams shows the same times draw by draw;
        maps whose physical chunks are co-located on purpose are reliably SLOW.  The discriminating counter is
        TCC_EA0_WRREQ_STALL (x 4.7 on a slow pair, concentrated in a few L2 channels) at identical request counts: the streams
        collide behind the L2, in the memory's own address mapping, which an unprivileged process can neither see nor choose.
        It can choose AGAIN, cheaply: the big map (most of the bytes) is kept, every other map is allocated anew -- behind a
        spacer, because the classes change every few tens of GiB -- ``steps`` steps are timed on each, the fastest set is kept.
        When three draws in a row have shown no contrast (within 2 %) the big map is drawn again as well, once per three draws.
        ``frames``: the caller's resident batch (its placement is part of the relation; ``placement="auto"`` tunes on the first batch
        ``step`` sees); default: synthetic noise.

        Bounds: ``tries`` draws incl. the first; ``budget_s`` seconds; ``spacer_gib`` per spacer, default AND upper limit = the size
        of the pipeline's maps; ``max_held_gib`` for everything the tuner holds at once (spacers + losing draws), default 16 x the
        maps, and never more than a quarter of the device or than leaves a quarter of it free.  Spacers and draws come from
        silent_malloc and go back to the driver at the end: torch's caching allocator is not involved and
        ``torch.cuda.empty_cache()`` is not called.  Results never depend on the choice.  The pipeline's map tensors are REPLACED:
        ``PackedPyramid`` views an earlier ``outputs()`` handed out keep pointing at the old buffers (alive, but no longer written)
        -- call ``outputs()`` again.  The decision is in ``placement_tuning``."""
        import time
        if self.attention and self._attention_state is self.energy:
            with self._parked_state():             # the timed steps run the tail on a scratch state: no stream advances
                return self.tune_placement(frames, tries, steps, budget_s, spacer_gib, max_held_gib)
        torch = self.torch
        if frames is None:
            frames = self._synthetic_frames()
        self._placement_pending = False
        self.wait()                                # nothing of an overlapped step in flight on the side streams
        torch.cuda.synchronize(self.tdev)
        was = self.overlap
        self.overlap = False
        t_start = time.perf_counter()
        for _ in range(20):                        # past the idle -> load transient of the chip
            self.step(frames)
        names = ("pyr", "cs", "end") if self.mode == "gray" else ("pyr", "orient", "line_end", "value")
        cur = {k: (self._pyrs[0] if k == "pyr" else getattr(self, k)) for k in names}
        if len(self._pyrs) > 1:                    # an overlapped pipeline alternates between two pyramid buffers: both are drawn
            cur["pyr1"] = self._pyrs[1]
        cur = {k: v for k, v in cur.items() if v is not None}
        nbytes = {k: v.numel() * v.element_size() for k, v in cur.items()}
        big = max(reversed([k for k in names if k in cur]), key=lambda k: nbytes[k])    # ties: the last written map (end / line_end)
        small = [k for k in cur if k != big]
        total_maps = sum(nbytes.values())
        spacer = total_maps if spacer_gib is None else min(int(spacer_gib * (1 << 30)), total_maps)
        free, total = torch.cuda.mem_get_info(self.tdev)
        cap = min(16 * total_maps, total // 4) if max_held_gib is None else int(max_held_gib * (1 << 30))
        best = (self._time_step(frames, steps), dict(cur))
        tried, drawn = [round(best[0], 4)], ["first"]
        held, held_bytes, stop, flat = [], 0, "tries", 0
        for i in range(tries - 1):
            if time.perf_counter() - t_start > budget_s:
                stop = "budget_s"
                break
            # no contrast in the last three draws: the small maps have not left their class -- move the big map too
            flat = flat + 1 if max(tried[-3:]) < 1.02 * min(tried[-3:]) else 0
            redraw = list(cur) if (flat >= 3 and len(tried) >= 3) else small
            if redraw is not small:
                flat = 0
            need = spacer + sum(nbytes[k] for k in redraw)
            free, total = torch.cuda.mem_get_info(self.tdev)
            if held_bytes + need > cap or free - need < total // 4:
                stop = "memory cap"
                break
            try:
                if spacer:
                    held.append(_RawBlock(self.ctx, spacer))
                cand = dict(best[1])
                cand.update({k: self._raw_tensor(cur[k]) for k in redraw})
            except RuntimeError:
                stop = "allocation failed"
                break
            held_bytes += need
            self._adopt_maps(cand)
            for _ in range(3):
                self.step(frames)
            t = self._time_step(frames, steps)
            tried.append(round(t, 4))
            drawn.append("all" if redraw is not small else "small")
            if t < best[0]:
                held.append(best[1])               # (tensors shared with ``cand`` stay alive through it)
                best = (t, cand)
            else:
                held.append(cand)
            del cand
        self._adopt_maps(best[1])
        torch.cuda.synchronize(self.tdev)
        held.clear()                               # spacers and losing draws: back to the driver (silent_free), not to a cache
        del cur
        self.overlap = was
        self.placement_tuning = {"tries_ms": tried, "drawn": drawn, "first_draw_ms": tried[0], "chosen_ms": round(best[0], 4),
                                 "big_map": big, "small_maps": small, "spacer_gib": round(spacer / (1 << 30), 2), "stopped_by": stop,
                                 "peak_held_gib": round(held_bytes / (1 << 30), 2), "seconds": round(time.perf_counter() - t_start, 2)}
        return self.placement_tuning

    def close(self):
        """Order the caller's stream and the host behind everything the pipeline has in flight on its own streams (overlap, ingest)
        before its buffers go back to the allocator: they were allocated on the constructor's stream, and the caching allocator
        would hand them to the next tensor of that stream while a side stream still writes them."""
        torch = getattr(self, "torch", None)
        if torch is None:
            return
        for st in (self._chain_stream, self._walk_stream, self._copy_stream):
            if st is not None:
                try:
                    st.synchronize()
                except Exception:          # (interpreter shutdown: the runtime may be gone)
                    pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _new_stream_pair(self, flip=False):
        """flip: the FIRST half's stream (pyramid / stream kernel) at the higher priority instead of the second half's."""
        torch = self.torch
        self._chain_stream = torch.cuda.Stream(self.tdev, priority=0 if flip else self._chain_priority)
        self._walk_stream, self.overlap_verified = pick_concurrent_stream(torch, self.tdev, [self._chain_stream],
                                                                         priority=self._chain_priority if flip else 0)
        self._pyr_ready = [torch.cuda.Event() for _ in range(2)]
        self._pyr_free = [None, None]
        self._steps = 0

    def tune_overlap(self, frames=None, candidates=8, steps=10, budget_s=3.0):
        """MEASURE whether two streams pay on this device, in this process, with these streams -- and with which.
        HIP multiplexes streams onto hardware queues (and those onto the command processor's pipes); which pair of streams a
        pipeline draws from the pool decides whether the pyramid of batch n + 1 really runs beside the chain of batch n (config 3:
        -10 %) or mostly waits on it through the cross-stream events (+0 ... +40 % on the small reference layout), and no static
        rule -- priorities, a concurrency check with independent busy-wait kernels -- predicts it (scripts/ab_overlap_pool.py).  So
        up to ``candidates`` pairs are timed on synthetic noise frames (``steps`` steps each, at most ``budget_s`` seconds in all)
        against the one-stream step; then the best pair and the one-stream step are timed AGAIN, alternately, three windows each
        (the minimum of eight candidates against a baseline timed twice is biased towards two streams), and the pair is kept only
        if that second measurement still wins by more than 2 %.  Otherwise the pipeline stays on one stream and the second
        pyramid buffer is released.  The decision is in ``overlap_tuning``.  Results never depend on the choice (bit-identical
        paths)."""
        if self.mode == "gray" and self.keypoints:
            raise ValueError("keypoints=True does not support overlap (the two-part gray step)")
        if self.attention:
            raise ValueError("attention=True does not support overlap (overlapped steps with the tail are not built)")
        import time
        torch = self.torch
        pending = self._placement_pending
        if pending and frames is not None:
            self.tune_placement(frames)            # first things first: which pair of streams pays depends on where the maps lie
            pending = False
        self._placement_pending = False            # (frames=None, the constructor's call: the placement waits for the caller's first batch)
        if frames is None:
            frames = self._synthetic_frames()
        t_start = time.perf_counter()
        self.wait()                                # (an overlapped step still in flight on the side streams: order it, then let it finish)
        torch.cuda.synchronize(self.tdev)
        if len(self._pyrs) < 2:
            self._pyrs.append(torch.empty_like(self._pyrs[0]))
        self.overlap = False
        for _ in range(30):                        # (past the idle -> load transient of the chip: a cold baseline flatters every candidate)
            self.step(frames)
        serial = self._time_step(frames, steps)
        tried, best = [], (None, None)
        for i in range(candidates):
            if time.perf_counter() - t_start > budget_s:
                break
            self._new_stream_pair(flip=bool(i & 1))         # (every other candidate with the priorities the other way round)
            self.overlap = True
            for _ in range(3):
                self.step(frames)
            t = self._time_step(frames, steps)
            tried.append(round(t, 4))
            if best[0] is None or t < best[0]:
                best = (t, (self._chain_stream, self._walk_stream, self.overlap_verified))
            torch.cuda.synchronize(self.tdev)
        # the decision: winner and baseline once more, alternately
        self.overlap = False
        self.pyr = self._pyrs[0]
        again_one, again_two = [], []
        if best[1] is not None and best[0] < 0.98 * serial:
            for _ in range(3):
                self.overlap = False
                self.pyr = self._pyrs[0]
                again_one.append(self._time_step(frames, steps, windows=1))
                self._new_stream_pair()
                self._chain_stream, self._walk_stream, self.overlap_verified = best[1]
                self.overlap = True
                for _ in range(3):
                    self.step(frames)
                again_two.append(self._time_step(frames, steps, windows=1))
                torch.cuda.synchronize(self.tdev)
            serial = min(again_one)
        keep = bool(again_two) and min(again_two) < 0.98 * min(again_one)
        if keep:
            self.overlap = True
        else:
            self.overlap = False
            self.pyr = self._pyrs[0]
            del self._pyrs[1:]                     # one stream: the second pyramid buffer (0.7 GB at config 2) is not held for nothing
            self._chain_stream = self._walk_stream = None
        torch.cuda.synchronize(self.tdev)
        self.overlap_tuning = {"one_stream_ms": round(serial, 4), "two_stream_candidates_ms": tried,
                               "remeasured_ms": {"one_stream": [round(t, 4) for t in again_one], "two_streams": [round(t, 4) for t in again_two]},
                               "chosen": "two streams" if self.overlap else "one stream",
                               "chosen_ms": round(min(again_two), 4) if self.overlap else round(serial, 4),
                               "stream_pair_verified_concurrent": self.overlap_verified if self.overlap else None,
                               "seconds": round(time.perf_counter() - t_start, 2)}
        self._placement_pending = pending
        return self.overlap_tuning

    # -- byte accounting -------------------------------------------------------
    def algorithmic_bytes_per_frame(self):
        """4*[H*W*C (frame read) + P*C (pyramid written) + P*C (pyramid read) + P*sum(C_out returned)]; for crop layouts the
        frame read is the largest crop any level resamples (the part of the frame the pyramid depends on).  storage="float16":
        the returned CS and end maps count 2 bytes per element.  frame_dtype="uint8": the frame read counts 1 byte per frame element
        ("uint16": 2 bytes) -- frame_shape[2] of them per pixel (3 for interleaved colour frames, whose pyramid and maps stay single-channel;
        mode "rgb" with rgb_frame_dtype="uint8" reports frame_dtype "uint8" and counts the same 1 byte per frame element; a strided
        view, frame_layout / rgb_frame_layout "strided", is read in place and counts the pixel bytes alone, not the bytes between them;
        rgb_frame_format="nv12" counts 1.5 bytes per pixel: the luma byte and half a chroma pair; "p010" / "p012" / "p016" 3 bytes per
        pixel: the luma element and half a pair of elements; "yuv420" / "yuv422" / "yuv444" 1 + 2 / 2^(sx + sy) bytes per pixel --
        1.5, 2 and 3: the luma byte and the pixel's share of a U and a V byte, whatever lies between them in a packed buffer not
        counted; the 16-bit triples of YUV16_FORMATS twice that -- 3, 4 and 6; a raw Bayer mosaic, "bayer_rggb" ..., 1 byte per pixel)."""
        h, w, fc = self.frame_shape
        c = self.channels
        if self.crop_px is not None:
            h, w = 1, self.crop_px
        # (rgb_storage="float16": a colour map's three channels cost 6 bytes per pixel -- 1.5 float32 channels; _map_bytes is 4 on mode "rgb")
        cc = 1.5 if self.rgb_storage == "float16" else 3
        outs = (1 + self.n_orient) if self.mode == "gray" else (cc + (cc if self.orient_map else 0) + (1 if self._value_written else 0))
        return int(self._frame_bytes * h * w * fc) + 4 * 2 * self.frame_px * c + int(self._map_bytes * self.frame_px * outs) + self.attention_bytes_per_frame()

    def attention_bytes_per_frame(self):
        """What the tail moves per frame (0 without attention=True): the value map read once and the half map's gathers (one value
        per half-map pixel); both distance maps written; per cell the state read twice and written once and the two cell results
        (C channels each) written.  The 8 + 8 + 4 + 4 bytes per cell of workspace between the two launches are not counted."""
        if not getattr(self, "attention", False):
            return 0
        half_px = sum(h * w for h, w in self.attention_half)
        return 4 * (2 * self.frame_px + 2 * half_px + self.cells_per_frame * (3 + 2 * self.attention_channels))

    @property
    def _value_written(self):
        """mode "rgb": the chain writes a float32 value map -- the kept one, or, with rgb_storage="float16" and selection, the one
        silent_rgb_keypoints_h keeps in the context workspace for its tail (the rounded colours do not give the value back)."""
        return self.value_map or (self.rgb_storage == "float16" and self.selection)

    @property
    def _map_bytes(self):
        """Bytes per element of the returned dense maps (not the pyramid)."""
        return 2 if self.storage == "float16" else 4

    @property
    def _frame_bytes(self):
        """Bytes per frame element as step() reads it (NV12: 1.5 bytes per pixel over the three channels; P010: 3 bytes per pixel)."""
        if self._source:                                             # elem (1 + 2 / 2^(sx + sy)) / 3: 0.5, 2 / 3, 1 -- 1, 4 / 3, 2 for uint16 -- exact
            src, sx, sy = self._source[:3]
            f = fractions.Fraction(src.elem * (2 ** (sx + sy) + 2), 3 * 2 ** (sx + sy))
            return float(f) if src.planes == 2 else f
        if self._bayer is not None:                                  # one byte per PIXEL over the three channels -- exact
            return fractions.Fraction(1, 3)
        return {"uint8": 1, "uint16": 2}.get(self.frame_dtype, 4)

    @property
    def _source(self):
        """(source description, sx, sy, depth, shift) of a mode "rgb" pipeline reading a YUV-family rgb_frame_format (_runtime.rgb_source:
        the one place that resolves the name), None for every other pipeline."""
        return _runtime.rgb_source(getattr(self, "rgb_frame_format", "interleaved"))

    @property
    def _nv12(self):
        """True for a mode "rgb" pipeline reading NV12 planes (rgb_frame_format="nv12")."""
        return getattr(self, "rgb_frame_format", "interleaved") == "nv12"

    @property
    def _p010(self):
        """The depth (10, 12, 16) of a mode "rgb" pipeline reading P010 / P012 / P016 planes, None for every other pipeline."""
        return _runtime.P010_DEPTHS.get(getattr(self, "rgb_frame_format", "interleaved"))

    @property
    def _yuv(self):
        """The chroma shifts (sx, sy) of a mode "rgb" pipeline reading a (y, u, v) triple ("yuv420" / "yuv422" / "yuv444"), else None."""
        return _runtime.YUV_SHIFTS.get(getattr(self, "rgb_frame_format", "interleaved"))

    @property
    def _yuv16(self):
        """(sx, sy, depth, shift) of a mode "rgb" pipeline reading a (y, u, v) triple of uint16 views (_runtime.YUV16_FORMATS), else None."""
        return _runtime.YUV16_FORMATS.get(getattr(self, "rgb_frame_format", "interleaved"))

    @property
    def _bayer(self):
        """The pattern (0 .. 3) of a mode "rgb" pipeline reading raw Bayer mosaics (_runtime.BAYER_FORMATS), else None."""
        return _runtime.BAYER_FORMATS.get(getattr(self, "rgb_frame_format", "interleaved"))

    @property
    def _frame_torch_dtype(self):
        """The torch dtype of the frames step() takes."""
        return getattr(self.torch, self.frame_dtype)

    @property
    def _colour_frames(self):
        """True for a gray pipeline reading interleaved 3-channel uint8 frames (frame_channels=3): the frame has more channels than
        the maps."""
        return self.mode == "gray" and self.frame_shape[2] == 3

    def filter_bytes_per_frame(self):
        """The filter pass alone: pyramid read once + every returned map written once."""
        c = self.channels
        # (rgb_storage="float16": a colour map's three channels cost 6 bytes per pixel -- 1.5 float32 channels; _map_bytes is 4 on mode "rgb")
        cc = 1.5 if self.rgb_storage == "float16" else 3
        outs = (1 + self.n_orient) if self.mode == "gray" else (cc + (cc if self.orient_map else 0) + (1 if self._value_written else 0))
        return int(self.frame_px * (4 * c + self._map_bytes * outs))

    def pyramid_bytes_per_frame(self):
        h, w, fc = self.frame_shape
        return int(self._frame_bytes * h * w * fc) + 4 * self.frame_px * self.channels

    def dominant_kernel_name(self):
        """Substring of the rocprofv3 kernel name of the launch that moves most bytes (bench.py matches PMC rows by it)."""
        return ("gray_stream_kernel<%d," % self.n_orient) if self.mode == "gray" else "rgb_line_end2_kernel"

    def launch_summary(self):
        if self.mode == "gray":
            return ("gray_stream_kernel (whole pyramid + level-0 CS/line-end, frame read once) + "
                    "gray_line_end_kernel (levels >= 1)" + (", float64 accumulation" if self.accumulation == "float64" else "")
                    + (", float16 CS / end maps" if self.storage == "float16" else "")
                    + (", %s frames" % self.frame_dtype if self.frame_dtype != "float32" else "")
                    + (" of 3 interleaved channels (value formed at the load)" if self._colour_frames else "")
                    + (", read in place from a strided view" if getattr(self, "frame_layout", "packed") == "strided" else ""))
        return ("single-read RGB pyramid (pyramid_walk3_kernel), fused RGB chain, max/min + fused selection "
                "(top 10 % > NMS > value), cell-max / count / scan / write keypoint kernels"
                + (", uint8 frames read in place (1 byte per frame element)" if getattr(self, "frame_dtype", "float32") == "uint8" else "")
                + (", read in place from a strided view" if getattr(self, "rgb_frame_layout", "packed") == "strided" else "")
                + self._source_summary()
                + (", attention tail (attn_cells_kernel + attn_pixels_kernel: centroids at two scales, boosting state per frame slot)"
                   if getattr(self, "attention", False) else ""))

    def _source_summary(self):
        """launch_summary's words on a YUV-family source: its planes and the bytes step() reads per pixel."""
        if self._bayer is not None:
            return ", %s mosaics read in place (one uint8 view, 1 byte per pixel, demosaiced in registers)" % self.rgb_frame_format
        if not self._source:
            return ""
        src = self._source[0]
        planes = ("uint16 Y + UV planes" if src.elem == 2 else "Y + UV planes") if src.planes == 2 else "a (y, u, v) triple of %s views" % src.dtype
        return ", %s read in place (%s, %s bytes per pixel, converted in registers)" % (
            self.rgb_frame_format.upper(), planes, ("%d" if src.elem == 2 else "%.1f") % (3 * self._frame_bytes))

    def _plane_shapes(self):
        """The shapes of the planes step() takes for a YUV-family source: (y, uv) of a pair, (y, u, v) of a triple."""
        src, sx, sy = self._source[:3]
        (h, w), b = self.frame_shape[:2], self.batch
        return ((b, h, w), (b, h // 2, w // 2, 2)) if src.planes == 2 else ((b, h, w),) + 2 * ((b, h >> sy, w >> sx),)

    # -- launches --------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.tdev).cuda_stream)

    def _source_arg(self, frames):
        """The const silent_<kind>_frames* of a pair (y, uv) / a triple (y, u, v) of GPU planes of this pipeline's batch (refused:
        anything else)."""
        src, sx, sy, depth, shift = self._source
        coeffs = (self.nv12_m, self.nv12_oy) + ((self.nv12_oc,) if src.elem == 2 else ())
        args, n, dev = _runtime.rgb_source_frames_of(src, frames, self.frame_shape[:2], coeffs, sx, sy, depth, shift, self.rgb_frame_format)
        if not dev or n != self.batch:
            shapes = [str(list(sh)) for sh in self._plane_shapes()]
            raise ValueError("frames must be a %s of %s GPU planes %s" % ("pair (y, uv)" if src.planes == 2 else "triple (y, u, v)", src.dtype,
                                                                          ", ".join(shapes[:-1]) + " and " + shapes[-1]))
        return getattr(_lib, src.kind + "_ptr")(args)

    def _bayer_arg(self, frames):
        """The const silent_bayer_frames* of a uint8 GPU view [batch, H, W] (or [batch, H, W, 1]) of this pipeline's batch (refused:
        anything else)."""
        (h, w), ok = self.frame_shape[:2], _runtime.is_torch_tensor(frames) and frames.is_cuda
        if ok:
            args, n, _ = _runtime.bayer_frames_of(frames, (h, w), self.rgb_frame_format, self.nv12_order)
            ok = n == self.batch
        if not ok:
            raise ValueError("frames must be a uint8 GPU tensor (any view with positive strides) of shape %s or %s"
                             % ((self.batch, h, w), (self.batch, h, w, 1)))
        return _lib.bayer_ptr(args)

    def _check_frames(self, frames):
        if getattr(self, "rgb_frame_layout", "packed") == "strided":
            shape = (self.batch,) + self.frame_shape
            if not _runtime.is_torch_tensor(frames) or tuple(frames.shape) != shape or frames.dtype != self.torch.uint8 or not frames.is_cuda:
                raise ValueError("frames must be a uint8 GPU tensor (any view with positive strides and channel stride 1) of shape %s" % (shape,))
            return
        if self.frame_layout == "strided":
            shapes = ((self.batch,) + self.frame_shape,) + (((self.batch,) + self.frame_shape[:2],) if self.frame_shape[2] == 1 else ())
            if not _runtime.is_torch_tensor(frames) or tuple(frames.shape) not in shapes or frames.dtype != self._frame_torch_dtype \
                    or not frames.is_cuda:
                raise ValueError("frames must be a %s GPU tensor (any view with positive strides) of shape %s" % (self.frame_dtype, shapes[0]))
            return
        want = self.torch.float32 if self.frame_dtype == "float32" else self._frame_torch_dtype
        if tuple(frames.shape) != (self.batch,) + self.frame_shape or frames.dtype != want \
                or not frames.is_cuda or not frames.is_contiguous():
            raise ValueError("frames must be a contiguous %s GPU tensor of shape %s" %
                             (self.frame_dtype, (self.batch,) + self.frame_shape,))

    def _frames_arg(self, frame_ptr, frames):
        """The frames argument of an entry point gray_entry chose: the view of a strided pipeline, the address otherwise."""
        if self.frame_layout == "strided":
            return frame_ptr(_runtime.frame_view_of(frames, self.frame_shape[2], self.frame_dtype))
        return frame_ptr(frames.data_ptr())

    def run_pyramid(self, frames, stream=None):
        if self._source:                                             # (mode "rgb", a YUV-family rgb_frame_format; the planes: _source_arg)
            entry = getattr(self._lib, "silent_pyramid_%s_dev" % self._source[0].kind)
            self.ctx.check(entry(self.ctx.handle, self.plan.handle, self._source_arg(frames), self.batch, C.c_void_p(self.pyr.data_ptr()),
                                 stream or self._stream()))
            return
        if self._bayer is not None:                                  # (mode "rgb", a raw Bayer mosaic: one uint8 GPU view)
            self.ctx.check(self._lib.silent_pyramid_bayer_dev(self.ctx.handle, self.plan.handle, self._bayer_arg(frames), self.batch,
                                                              C.c_void_p(self.pyr.data_ptr()), stream or self._stream()))
            return
        self._check_frames(frames)
        if getattr(self, "rgb_frame_layout", "packed") == "strided":   # (mode "rgb", rgb_frame_dtype="uint8")
            self.ctx.check(self._lib.silent_pyramid_rgb8_view_dev(self.ctx.handle, self.plan.handle,
                                                                  _lib.view_ptr(_runtime.frame_view_of(frames, 3, "uint8")), self.batch,
                                                                  C.c_void_p(self.pyr.data_ptr()), stream or self._stream()))
            return
        if self.mode == "rgb" and self.frame_dtype == "uint8":     # (rgb_frame_dtype="uint8")
            self.ctx.check(self._lib.silent_pyramid_rgb8_dev(self.ctx.handle, self.plan.handle, _lib.byte_ptr(frames.data_ptr()),
                                                             self.batch, C.c_void_p(self.pyr.data_ptr()), stream or self._stream()))
            return
        if self.frame_dtype == "uint16":
            name, frame_ptr, _, _ = _lib.gray_entry("pyramid", "uint16", frame_layout=self.frame_layout)
            self.ctx.check(getattr(self._lib, "silent_" + name + "_dev")(self.ctx.handle, self.plan.handle, self._frames_arg(frame_ptr, frames),
                                                                         self.batch, C.c_void_p(self.pyr.data_ptr()), stream or self._stream()))
            return
        if self.frame_layout == "strided":
            self.ctx.check(self._lib.silent_pyramid_view_dev(self.ctx.handle, self.plan.handle, self._frames_arg(_lib.view_ptr, frames),
                                                             self.batch, C.c_void_p(self.pyr.data_ptr()), stream or self._stream()))
            return
        if self.frame_dtype == "uint8":
            fn = self._lib.silent_pyramid_u8x3_dev if self._colour_frames else self._lib.silent_pyramid_u8_dev
            self.ctx.check(fn(self.ctx.handle, self.plan.handle, _lib.byte_ptr(frames.data_ptr()),
                                                           self.batch, C.c_void_p(self.pyr.data_ptr()), stream or self._stream()))
            return
        self.ctx.check(self._lib.silent_pyramid_dev(self.ctx.handle, self.plan.handle, C.c_void_p(frames.data_ptr()),
                                                    self.batch, C.c_void_p(self.pyr.data_ptr()),
                                                    stream or self._stream()))

    def run_filters(self, stream=None):
        s = stream or self._stream()
        if self.mode == "gray":
            if self.storage == "float16":
                raise ValueError("storage='float16' has no per-op filter pass (silent_gray_line_end writes float32): use run_gray_pass")
            self.ctx.check(self._lib.silent_gray_line_end_dev(
                self.ctx.handle, C.c_void_p(self.pyr.data_ptr()), self.levels_c, self.n_levels, self.batch,
                C.c_void_p(self.consts["cs"].ctypes.data), C.c_void_p(self.consts["end"].ctypes.data), self.n_orient,
                self.clip_hi, C.c_void_p(self.cs.data_ptr()), C.c_void_p(self.end.data_ptr()), s))
        else:
            if self.rgb_storage == "float16":
                raise ValueError("rgb_storage='float16' has no per-op filter pass (silent_rgb_line_end writes float32): use run_chain_h")
            self.ctx.check(self._lib.silent_rgb_line_end_dev(
                self.ctx.handle, C.c_void_p(self.pyr.data_ptr()), self.levels_c, self.n_levels, self.batch,
                C.byref(self._params), C.c_void_p(self.orient.data_ptr()) if self.orient is not None else None,
                C.c_void_p(self.line_end.data_ptr()),
                C.c_void_p(self.value.data_ptr()) if self.value is not None else None, s))

    def run_filters_keypoints(self, stream=None):
        """rgb, selection without the intermediate colour maps: chain + a-10 -> a-9 -> a-8 -> a-11 in one C-ABI call
        (silent_rgb_keypoints_dev): the chain kernel accumulates the per-level extrema of a-10 itself."""
        if self.rgb_storage == "float16":
            raise ValueError("rgb_storage='float16' has no float32 fused step (silent_rgb_keypoints writes float32 maps into buffers of half "
                             "the size): use run_chain_h")
        s = stream or self._stream()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self.ctx.check(self._lib.silent_rgb_keypoints_dev(
            self.ctx.handle, p(self.pyr), self.levels_c, self.n_levels, self.batch, C.byref(self._params), self.top_percent,
            self.regions, p(self.orient), p(self.line_end), p(self.value), p(self.peak_value), p(self.kp_idx), self.kp_cap,
            p(self.kp_counts), s))

    def run_chain_h(self, stream=None):
        """rgb, rgb_storage="float16": the chain with float16 orient / line_end maps and the keypoints.  selection=True:
        silent_rgb_keypoints_h_dev (chain + selection tail in one call); selection=False: silent_rgb_line_end_h_dev, then the
        keypoints from the float32 value map (silent_max_value_indices_region_dev) -- the float32 pipeline's, bit for bit."""
        s = stream or self._stream()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        h = lambda t: _lib.half_ptr(t.data_ptr()) if t is not None else None
        geom = (self.levels_c, self.n_levels, self.batch)
        if self.selection:
            self.ctx.check(self._lib.silent_rgb_keypoints_h_dev(
                self.ctx.handle, p(self.pyr), *geom, C.byref(self._params), self.top_percent, self.regions, h(self.orient),
                h(self.line_end), p(self.value), p(self.peak_value), p(self.kp_idx), self.kp_cap, p(self.kp_counts), s))
            return
        self.ctx.check(self._lib.silent_rgb_line_end_h_dev(
            self.ctx.handle, p(self.pyr), *geom, C.byref(self._params), h(self.orient), h(self.line_end), p(self.value), s))
        self.ctx.check(self._lib.silent_max_value_indices_region_dev(
            self.ctx.handle, p(self.value), *geom, self.regions, p(self.kp_idx), self.kp_cap, p(self.kp_counts), s))

    def sparse_tail_stats(self):
        """What the sparse keypoint tail of the last fused step did: dict(ran, pairs, dense_pairs, candidates)."""
        st = (C.c_int64 * 5)()
        self.ctx.check(self._lib.silent_sparse_tail_stats(self.ctx.handle, st))
        return {"ran": bool(st[0]), "pairs": int(st[1]), "dense_pairs": int(st[2]), "zero_map_pairs": int(st[4]),
                "candidates": int(st[3])}

    def run_keypoints(self, stream=None):
        if self.rgb_storage == "float16":
            raise ValueError("rgb_storage='float16' has no per-op keypoint pass (the per-op kernels read float32 maps): use run_chain_h")
        s = stream or self._stream()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # (no value map: the selection takes it from line_end)
        geom = (self.levels_c, self.n_levels, self.batch)
        if self.selection and not self.keep_selection_maps:
            # a-10 -> a-9 -> a-8 -> a-11 as one composite: the keypoint search's cell maxima come out of the selection pass
            self.ctx.check(self._lib.silent_select_keypoints_dev(
                self.ctx.handle, p(self.line_end), p(self.value), *geom, 3, self.top_percent, self.regions,
                p(self.peak_value), p(self.kp_idx), self.kp_cap, p(self.kp_counts), s))
            return
        value = self.value
        if self.selection:
            # the same with the two intermediate colour maps kept (tests, visualisation)
            self.ctx.check(self._lib.silent_select_peaks_dev(
                self.ctx.handle, p(self.line_end), p(self.value), *geom, 3, self.top_percent, p(self.top), p(self.peaks),
                p(self.peak_value), s))
            value = self.peak_value
        self.ctx.check(self._lib.silent_max_value_indices_region_dev(
            self.ctx.handle, p(value), *geom, self.regions, p(self.kp_idx), self.kp_cap, p(self.kp_counts), s))

    def run_gray_keypoints(self, frames, stream=None):
        """gray, keypoints=True: the whole pass + the keypoint tail in one C-ABI call (silent_gray_keypoints_dev): the kernels that
        write the end map fold the padded value map into what the tail needs; pyramid / cs / end are those of run_gray_pass."""
        self._check_frames(frames)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        name, frame_ptr, _, _ = _lib.gray_entry("gray_keypoints", self.frame_dtype, self.frame_shape[2], dev=True,
                                                frame_layout=self.frame_layout)
        fn, fp = getattr(self._lib, "silent_" + name + "_dev"), self._frames_arg(frame_ptr, frames)
        self.ctx.check(fn(
            self.ctx.handle, self.plan.handle, fp, self.batch, C.c_void_p(self.consts["cs"].ctypes.data),
            C.c_void_p(self.consts["end"].ctypes.data), self.n_orient, self.clip_hi, p(self.pyr), p(self.cs), p(self.end), self.pad,
            int(self.selection), self.top_percent, self.regions, p(self.value), p(self.peak_value), p(self.kp_idx), self.kp_cap,
            p(self.kp_counts), stream or self._stream()))

    def run_gray_pass(self, frames, stream=None, parts=3):
        """Whole grayscale hot path in one C-ABI call (silent_gray_pass_dev): region kernel for the non-unit
        levels, fused pyramid + CS + end kernel for the unit levels, filter kernel for the rest.  ``parts``: 1 = pyramid + unit
        levels only, 2 = the filter of the remaining levels only (silent_gray_pass_parts_dev; the halves of an overlapped step)."""
        self._check_frames(frames)
        name, frame_ptr, map_ptr, tail = _lib.gray_entry("gray_pass", self.frame_dtype, self.frame_shape[2], self.storage, True, parts,
                                                         frame_layout=self.frame_layout)
        self.ctx.check(getattr(self._lib, "silent_" + name + "_dev")(
            self.ctx.handle, self.plan.handle, self._frames_arg(frame_ptr, frames), self.batch, C.c_void_p(self.consts["cs"].ctypes.data),
            C.c_void_p(self.consts["end"].ctypes.data), self.n_orient, self.clip_hi, C.c_void_p(self.pyr.data_ptr()),
            map_ptr(self.cs.data_ptr()), map_ptr(self.end.data_ptr()), *(tail + (stream or self._stream(),))))

    def set_profiling(self, every=1):
        """Bracket the dominant kernel with HIP events on every ``every``-th step (0 / False: off)."""
        self.ctx.check(self._lib.silent_set_profiling(self.ctx.handle, int(every)))

    def profiled_kernel(self):
        """(milliseconds, pixels) of the dominant kernel of the last run_gray_pass (HIP events on its stream)."""
        ms, px = C.c_float(0), C.c_int64(0)
        self.ctx.check(self._lib.silent_profile_elapsed_ms(self.ctx.handle, C.byref(ms), C.byref(px)))
        return ms.value, px.value

    def _step_overlapped(self, frames):
        torch = self.torch
        k = self._steps & 1
        self._steps += 1
        self.pyr = self._pyrs[k]
        ws, cs = self._walk_stream, self._chain_stream
        ws.wait_stream(torch.cuda.current_stream(self.tdev))     # the frames were produced on the caller's stream
        if self._pyr_free[k] is not None:
            ws.wait_event(self._pyr_free[k])                      # the chain of two steps ago has read this buffer
        if self.mode == "gray":
            self.run_gray_pass(frames, C.c_void_p(ws.cuda_stream), parts=_lib.GRAY_PART_PYRAMID)
        else:
            self.run_pyramid(frames, C.c_void_p(ws.cuda_stream))
        self._pyr_ready[k].record(ws)
        cs.wait_event(self._pyr_ready[k])
        # the caller's stream is ordered behind the READ of its frames (not behind the chain): whatever it enqueues next may
        # overwrite them, exactly as after a one-stream step
        if self._order_caller:
            torch.cuda.current_stream(self.tdev).wait_event(self._pyr_ready[k])
        s = C.c_void_p(cs.cuda_stream)
        if self.mode == "gray":
            self.run_gray_pass(frames, s, parts=_lib.GRAY_PART_FILTER)
        elif self.rgb_storage == "float16":
            self.run_chain_h(s)
        elif self.selection and not self.keep_selection_maps:
            self.run_filters_keypoints(s)
        else:
            self.run_filters(s)
            self.run_keypoints(s)
        if self._pyr_free[k] is None:
            self._pyr_free[k] = torch.cuda.Event()
        self._pyr_free[k].record(cs)

    def wait(self):
        """Order the caller's current stream behind everything step() has enqueued (a no-op without ``overlap``)."""
        if self.overlap:
            cur = self.torch.cuda.current_stream(self.tdev)
            cur.wait_stream(self._chain_stream)
            cur.wait_stream(self._walk_stream)

    # -- ingest: host frames -> pinned ring -> copy stream -> widening cast -> step -----------------------------
    def _ingest_slot(self, dtype, pinned_source):
        """Ring of two slots per dtype: [pinned staging buffer (None when the caller's frames are pinned already), device buffer
        of the source dtype, float32 frame buffer, events].  Two batches are in flight: while batch n computes, batch n + 1 is
        copied (and, for NumPy sources, batch n + 2 staged by the host).  A uint8 / uint16 pipeline's slots have no float32 frame
        buffer: step() reads the uint8 / uint16 device buffer itself."""
        torch = self.torch
        ring = self._ingest.setdefault(dtype, {"slots": [], "next": 0})
        if not ring["slots"]:
            shape = (self.batch,) + self.frame_shape
            for _ in range(2):
                ring["slots"].append({
                    "pinned": None,
                    "raw": torch.empty(shape, dtype=dtype, device=self.tdev) if dtype != torch.float32 else None,
                    "f32": torch.empty(shape, dtype=torch.float32, device=self.tdev) if self.frame_dtype == "float32" else None,
                    "h2d_done": torch.cuda.Event(), "raw_free": None, "f32_free": None})
        slot = ring["slots"][ring["next"]]
        ring["next"] ^= 1
        if not pinned_source and slot["pinned"] is None:
            slot["pinned"] = torch.empty((self.batch,) + self.frame_shape, dtype=dtype, pin_memory=True)
        return slot

    def step_host(self, frames):
        """One pass over a batch of HOST frames -- the reference's per-call ingest, recognition_testing.py:141-143
        (np.asarray(frame, float32) -> zoom.from_image -> session.run feed), batched: ``frames`` [batch, H, W, C] as a NumPy array
        or a CPU torch tensor (uint8 as a camera delivers it, or int16 / uint16 / int32 / float32 / float64).  The batch goes
        through a pinned staging buffer (skipped when ``frames`` is a pinned torch tensor already), an asynchronous host-to-device
        copy on the pipeline's COPY stream, the library's widening cast (silent_cast_interleave_dev: uint8 -> float32 on the GPU,
        a quarter of the PCIe bytes) and step().  Returns at once; two batches are in flight (ring of two slots), so the copy of
        batch n + 1 overlaps the compute of batch n.  Results are bit-identical to step() on the same frames resident as float32.
        A frame_dtype="uint8" pipeline takes uint8 host frames only: staging -> copy into the slot's uint8 device buffer -> step();
        no cast launch and no float32 frame buffer.  A frame_dtype="uint16" pipeline likewise takes uint16 host frames only, and a
        mode "rgb" pipeline with rgb_frame_dtype="uint8" uint8 host frames [batch, H, W, 3] only; one reading raw Bayer mosaics
        (rgb_frame_format="bayer_rggb" ...) a uint8 NumPy array [batch, H, W] or [batch, H, W, 1] (_step_host_bayer)."""
        torch = self.torch
        if self._source:
            return self._step_host_nv12(frames)
        if self._bayer is not None:
            return self._step_host_bayer(frames)
        if isinstance(frames, np.ndarray):
            src = torch.from_numpy(np.ascontiguousarray(frames))
        else:
            src = frames.contiguous()
        if src.is_cuda or tuple(src.shape) != (self.batch,) + self.frame_shape:
            raise ValueError("step_host takes host frames of shape %s" % ((self.batch,) + self.frame_shape,))
        if self.frame_dtype != "float32":
            if src.dtype != self._frame_torch_dtype:
                raise ValueError("step_host of a frame_dtype='%s' pipeline takes %s host frames, got %s"
                                 % (self.frame_dtype, self.frame_dtype, src.dtype))
        elif src.dtype != torch.float32:
            _runtime._torch_dtype_code(src)         # TypeError for dtypes the cast kernel does not take
        cs = self._copy_stream_of_the_ingest()
        pinned_source = src.is_pinned()
        slot = self._ingest_slot(src.dtype, pinned_source)
        cur = torch.cuda.current_stream(self.tdev)
        if not pinned_source:
            slot["h2d_done"].synchronize()          # the staging buffer's previous copy has left the host
            _staging_copy(slot["pinned"], src)
            src = slot["pinned"]
        if self.frame_dtype != "float32":
            # the frame-reading kernels read the uint8 / uint16 device buffer itself: it is free again where THEY finish -- on the walk stream
            # with overlap, else on the caller's stream (where a float32 pipeline records f32_free)
            if slot["raw_free"] is not None:
                cs.wait_event(slot["raw_free"])     # the previous batch of this slot has been read on the device
            with torch.cuda.stream(cs):
                slot["raw"].copy_(src, non_blocking=True)
            slot["h2d_done"].record(cs)
            cur.wait_event(slot["h2d_done"])
            self.step(slot["raw"])
            if slot["raw_free"] is None:
                slot["raw_free"] = torch.cuda.Event()
            slot["raw_free"].record(self._walk_stream if self.overlap else cur)
            return
        dst = slot["f32"] if slot["raw"] is None else slot["raw"]
        for ev in ((slot["f32_free"],) if slot["raw"] is None else (slot["raw_free"],)):
            if ev is not None:
                cs.wait_event(ev)                   # the previous batch of this slot has been consumed on the device
        with torch.cuda.stream(cs):
            dst.copy_(src, non_blocking=True)
        slot["h2d_done"].record(cs)
        cur.wait_event(slot["h2d_done"])
        if slot["raw"] is not None:
            if slot["f32_free"] is not None:
                cur.wait_event(slot["f32_free"])
            c = self.channels
            _runtime.cast_interleave(slot["raw"], slot["f32"], c, 0, c, c, 0, self.batch * self.frame_shape[0] * self.frame_shape[1])
            if slot["raw_free"] is None:
                slot["raw_free"] = torch.cuda.Event()
            slot["raw_free"].record(cur)
        self.step(slot["f32"])
        # the float32 frames are read by the pyramid kernel only: on the walk stream with overlap, else on the caller's stream
        if slot["f32_free"] is None:
            slot["f32_free"] = torch.cuda.Event()
        slot["f32_free"].record(self._walk_stream if self.overlap else cur)

    def _copy_stream_of_the_ingest(self):
        """The copy stream of step_host, made with the ingest ring on the first call."""
        torch = self.torch
        if not hasattr(self, "_ingest"):
            # a stream of another priority than the compute stream gets a hardware queue of its own (two equal-priority streams
            # may share one, and then copy and compute do not overlap): -1 beside a caller's normal stream; with overlap=True the
            # chain stream holds -1 and the copies queue with the pyramid stream, which has to follow them anyway
            self._ingest = {}
            beside = [self._chain_stream, self._walk_stream] if self.overlap else [torch.cuda.current_stream(self.tdev)]
            self._copy_stream, self.copy_stream_verified = pick_concurrent_stream(torch, self.tdev, beside, priority=0 if self.overlap else -1)
        return self._copy_stream

    def _step_host_nv12(self, frames):
        """step_host of an rgb_frame_format="nv12" pipeline: ``frames`` is the pair (y [batch, H, W], uv [batch, H / 2, W / 2, 2]) as
        uint8 NumPy arrays (any pitch: the staging copy packs).  Both planes go through pinned staging buffers and asynchronous copies
        on the copy stream into a ring of two device slots, which step() reads in place; no cast, no conversion launch."""
        torch = self.torch
        # (a triple: three planes of any strides in the ring, packed by the staging copy; uint16 sources: the same ring with uint16 planes)
        src, shapes = self._source[0], self._plane_shapes()
        np_dtype, t_dtype = np.dtype(src.dtype).type, getattr(torch, src.dtype)
        if not isinstance(frames, (tuple, list)) or len(frames) != len(shapes) or any(
                not isinstance(p, np.ndarray) or p.dtype != np_dtype or tuple(p.shape) != sh for p, sh in zip(frames, shapes)):
            raise ValueError("step_host of an rgb_frame_format=%r pipeline takes a %s of %s arrays of shapes %s"
                             % (self.rgb_frame_format, "triple" if src.planes == 3 else "pair", src.dtype,
                                " and ".join(str(sh) for sh in shapes)))
        self._step_host_planes("nv12", frames, shapes, t_dtype, lambda raw: tuple(raw))

    def _step_host_planes(self, key, planes, shapes, t_dtype, frames_of):
        """The ingest of host planes that step() reads in place (the YUV family's pair / triple, a Bayer mosaic): each plane through a
        pinned staging buffer and an asynchronous copy on the copy stream into ring ``key`` of two device slots; step(frames_of(the
        slot's device planes)); the slot is free again where the frame-reading kernels finish."""
        torch = self.torch
        cs = self._copy_stream_of_the_ingest()
        ring = self._ingest.setdefault(key, {"slots": [], "next": 0})
        if not ring["slots"]:
            for _ in range(2):
                ring["slots"].append({"pinned": [torch.empty(sh, dtype=t_dtype, pin_memory=True) for sh in shapes],
                                      "raw": [torch.empty(sh, dtype=t_dtype, device=self.tdev) for sh in shapes],
                                      "h2d_done": torch.cuda.Event(), "raw_free": None})
        slot = ring["slots"][ring["next"]]
        ring["next"] ^= 1
        cur = torch.cuda.current_stream(self.tdev)
        slot["h2d_done"].synchronize()              # the staging buffers' previous copies have left the host
        for pin, p in zip(slot["pinned"], planes):
            _staging_copy(pin, torch.from_numpy(np.ascontiguousarray(p)))
        if slot["raw_free"] is not None:
            cs.wait_event(slot["raw_free"])         # the previous batch of this slot has been read on the device
        with torch.cuda.stream(cs):
            for raw, pin in zip(slot["raw"], slot["pinned"]):
                raw.copy_(pin, non_blocking=True)
        slot["h2d_done"].record(cs)
        cur.wait_event(slot["h2d_done"])
        self.step(frames_of(slot["raw"]))
        if slot["raw_free"] is None:
            slot["raw_free"] = torch.cuda.Event()
        slot["raw_free"].record(self._walk_stream if self.overlap else cur)

    def _step_host_bayer(self, frames):
        """step_host of a Bayer pipeline: ``frames`` is the mosaic batch [batch, H, W] (or [batch, H, W, 1]) as a uint8 NumPy array (any
        strides: the staging copy packs).  It goes through a pinned staging buffer and an asynchronous copy on the copy stream into a
        ring of two device slots of MOSAICS, 1 B/px, which step() reads in place; no cast, no demosaic launch."""
        torch = self.torch
        shape = (self.batch,) + self.frame_shape[:2]
        if isinstance(frames, np.ndarray) and frames.ndim == 4 and frames.shape[3] == 1:
            frames = frames[..., 0]
        if not isinstance(frames, np.ndarray) or frames.dtype != np.uint8 or tuple(frames.shape) != shape:
            raise ValueError("step_host of an rgb_frame_format=%r pipeline takes a uint8 array of shape %s or %s"
                             % (self.rgb_frame_format, shape, shape + (1,)))
        self._step_host_planes("bayer", [frames], [shape], torch.uint8, lambda raw: raw[0])

    def step(self, frames):
        """One pass of the hot path over one batch of frames (asynchronous)."""
        if self._placement_pending:
            self.tune_placement(frames)            # once, on the first batch (placement="auto")
        if self.overlap:
            return self._step_overlapped(frames)
        s = self._stream()
        if self.mode == "gray":
            if self.keypoints:
                self.run_gray_keypoints(frames, s)
            else:
                self.run_gray_pass(frames, s)
            return
        self.run_pyramid(frames, s)
        if self.rgb_storage == "float16":
            self.run_chain_h(s)
        elif self.selection and not self.keep_selection_maps:
            self.run_filters_keypoints(s)
        else:
            self.run_filters(s)
            self.run_keypoints(s)
        if self.attention:
            self.run_attention(s)

    # -- results as PackedPyramids over the pipeline's buffers ---------------------------------------
    def outputs(self, allow_truncated=False):
        """Views over the pipeline's buffers (maps) and host copies of the keypoints.  Raises ValueError when a frame
        produced more keypoints than ``max_keypoints_per_frame`` (like the host entry point's SILENT_E_CAPACITY) unless
        ``allow_truncated``; ``keypoint_counts`` always holds the true counts."""
        P = _runtime.PackedPyramid
        self.wait()
        out = {"pyramid": P(self.pyr, self.extents, self.channels, self.batch)}
        if self.mode == "gray":
            dt = np.float16 if self.storage == "float16" else np.float32
            out["cs"] = P(self.cs, self.extents, 1, self.batch, dtype=dt)
            out["end"] = P(self.end, self.extents, self.n_orient, self.batch, dtype=dt)
            if self.keypoints:
                for name in ("value", "peak_value"):
                    if getattr(self, name) is not None:
                        out[name] = P(getattr(self, name), self.extents, 1, self.batch)
                self._keypoint_outputs(out, allow_truncated)
        else:
            dt = np.float16 if self.rgb_storage == "float16" else np.float32
            if self.orient is not None:
                out["orient"] = P(self.orient, self.extents, 3, self.batch, dtype=dt)
            out["line_end"] = P(self.line_end, self.extents, 3, self.batch, dtype=dt)
            if self.value_map:
                out["value"] = P(self.value, self.extents, 1, self.batch)
            if self.selection:
                if self.keep_selection_maps:
                    out["top"] = P(self.top, self.extents, 3, self.batch)
                    out["peaks"] = P(self.peaks, self.extents, 3, self.batch)
                if self.peak_value is not None:
                    out["peak_value"] = P(self.peak_value, self.extents, 1, self.batch)
            if self.attention:
                c = self.attention_channels
                out["centroids"] = P(self.centroids, self.extents, 1, self.batch)
                out["centroids2"] = P(self.centroids2, self.attention_half, 1, self.batch)
                out["fired"] = P(self.fired, self.attention_cells, c, self.batch)
                out["update"] = P(self.update, self.attention_cells, c, self.batch)
            self._keypoint_outputs(out, allow_truncated)
        return out

    def _keypoint_outputs(self, out, allow_truncated):
        """keypoints / keypoint_counts into ``out`` (host copies of the rows each frame produced)."""
        counts = self.kp_counts.cpu().numpy()
        if not allow_truncated and (counts > self.kp_cap).any():
            # the asynchronous *_dev entry points cannot return SILENT_E_CAPACITY: counts[f] > cap IS the overflow flag
            raise ValueError("keypoint capacity exceeded: frame %d produced %d rows, max_keypoints_per_frame is %d "
                             "(only the first %d were written; pass allow_truncated=True to take them)"
                             % (int(np.argmax(counts)), int(counts.max()), self.kp_cap, self.kp_cap))
        # (only the rows each frame produced: the buffer holds kp_cap rows per frame -- every pyramid pixel by default)
        out["keypoints"] = [self.kp_idx[f, :min(int(counts[f]), self.kp_cap)].cpu().numpy() for f in range(self.batch)]
        out["keypoint_counts"] = counts
        return out
