"""Host-side runtime above the C ABI: contexts, tensor adapters, one thin wrapper per entry point.

Tensors the wrappers accept (the reference accepts ``tf.Tensor`` or ``np.ndarray``, get_dimensions.py:9-12):
  * ``np.ndarray`` rank 4 NHWC  -> host-pointer entry points, result is a fresh float32 ndarray
  * ``torch.Tensor`` on a ROCm device, rank 4 NHWC -> ``*_dev`` entry points on torch's current stream,
    result is a torch tensor on the same device (PyTorch is only the allocator / stream provider)
  * ``PackedPyramid`` (ragged levels, host or device) -> same, result is a PackedPyramid
Anything else raises the reference's TypeError.
"""
import collections
import ctypes as C
import os

import weakref

import numpy as np

from . import _lib

TYPE_ERROR_MESSAGE = "Input to orientation filter must either be tensor or numpy array."


# ----------------------------------------------------------------------------- context

class Context(object):
    """One silent_ctx: one per (host thread, GPU); not thread-safe."""

    def __init__(self, device=0):
        lib = _lib.load()
        self._lib = lib
        self.device = int(device)
        self.handle = C.c_void_p()
        rc = lib.silent_create(self.device, C.byref(self.handle))
        if rc != _lib.SILENT_OK:
            msg = _lib.last_error(None)
            self.handle = C.c_void_p()
            raise RuntimeError("pysilent_amd needs an MI355X (gfx950) GPU and has no CPU fallback: " + msg)

    @property
    def name(self):
        buf = C.create_string_buffer(256)
        self._lib.silent_device_name(self.handle, buf, 256)
        return buf.value.decode()

    def check(self, rc):
        _lib.check(rc, self.handle)

    def set_tuning(self, which, value):
        """Kernel-selection knob of this context (silent_set_tuning): _lib.TUNE_GRAY / TUNE_RGB / TUNE_PYRAMID."""
        self.check(self._lib.silent_set_tuning(self.handle, int(which), C.c_uint(int(value))))

    def get_tuning(self, which):
        v = C.c_uint(0)
        self.check(self._lib.silent_get_tuning(self.handle, int(which), C.byref(v)))
        return int(v.value)

    def close(self):
        if self.handle:
            self._lib.silent_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts = {}


def default_device():
    if "SILENT_DEVICE" in os.environ:
        return int(os.environ["SILENT_DEVICE"])
    return int(os.environ.get("LOCAL_RANK", "0"))


_override = []      # stack of private contexts (use_context)


class use_context(object):
    """``with use_context(ctx): ...`` -- every op inside runs on ``ctx`` instead of the shared per-device context.
    A caller that bakes device pointers into a HIP graph needs this: the workspace of its private context only
    grows for its own calls, so what the graph captured stays valid."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        _override.append(self.ctx)
        return self.ctx

    def __exit__(self, *exc):
        _override.pop()
        return False


def get_context(device=None):
    device = default_device() if device is None else int(device)
    if _override and _override[-1].device == device:
        return _override[-1]
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = Context(device)
    return ctx


class tuning(object):
    """``with tuning(TUNE_RGB, 1): ...`` -- run the ops inside with a kernel-selection knob of the current context set."""

    def __init__(self, which, value, device=None):
        self.which, self.value, self.device = which, value, device

    def __enter__(self):
        self.ctx = get_context(self.device)
        self.old = self.ctx.get_tuning(self.which)
        self.ctx.set_tuning(self.which, self.value)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_tuning(self.which, self.old)
        return False


def device_count():
    n = C.c_int(0)
    _lib.load().silent_device_count(C.byref(n))
    return n.value


# ----------------------------------------------------------------------------- tensors

def is_torch_tensor(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _torch_dtype_code(t):
    import torch
    table = {torch.uint8: _lib.DT_U8, torch.float32: _lib.DT_F32, torch.float64: _lib.DT_F64, torch.int32: _lib.DT_I32,
             torch.int16: _lib.DT_I16, torch.int64: _lib.DT_I64}
    if hasattr(torch, "uint16"):
        table[torch.uint16] = _lib.DT_U16
    if t.dtype not in table:
        raise TypeError("unsupported tensor dtype %s (uint8, int16, int32, int64, float32, float64)" % t.dtype)
    return table[t.dtype]


def cast_interleave(src, out, in_stride, in_offset, count, out_stride, out_offset, n_pixels):
    """out[p * out_stride + out_offset + k] = float32(src[p * in_stride + in_offset + k]) on the GPU (silent_cast_interleave_dev,
    torch's current stream): dtype widening, cutting a colour plane out of an interleaved image, interleaving planes."""
    import torch
    ctx = get_context(src.device.index or 0)
    stream = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    ctx.check(_lib.load().silent_cast_interleave_dev(ctx.handle, C.c_void_p(src.data_ptr()), _torch_dtype_code(src), int(n_pixels),
                                                    int(in_stride), int(in_offset), int(count), C.c_void_p(out.data_ptr()),
                                                    int(out_stride), int(out_offset), stream))
    return out


def as_float32(t):
    """A contiguous float32 GPU tensor with the values of ``t`` (np.asarray(frame, dtype=float32) of
    recognition_testing.py:141 for device tensors: any layout, any dtype).  float32 contiguous tensors pass through; contiguous
    uint8 / int16 / uint16 / int32 / int64 / float64 tensors are widened by the library's own cast kernel (the fast path: no
    torch kernel); anything else -- a strided view such as ``x.permute(...)`` or ``x[..., :3]``, float16 / bfloat16 / bool /
    int8 -- is made contiguous float32 by torch first, like ``tensor.to(float32).contiguous()`` did before round 3."""
    import torch
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    try:
        code_ok = t.is_contiguous() and _torch_dtype_code(t) is not None
    except TypeError:
        code_ok = False
    if not code_ok:
        return t.to(torch.float32).contiguous()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    if t.numel():
        cast_interleave(t, out, 1, 0, 1, 1, 0, t.numel())
    return out


class PackedPyramid(object):
    """A batch of pyramids with per-level extents, packed as the C ABI wants it.

    ``data`` is a flat float32 buffer (np.ndarray, or torch tensor on the GPU) of
    ``n_frames * sum(h_l * w_l) * channels`` elements: frames outermost, then levels, NHWC inside.  ``dtype``: np.float32, or
    np.float16 for the CS / end maps of a gray pass with storage="float16" (a torch buffer keeps its own dtype)."""

    def __init__(self, data, extents, channels, n_frames=1, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
            raise ValueError("PackedPyramid: dtype must be float32 or float16, got %s" % (self.dtype,))
        self.extents = [(int(h), int(w)) for h, w in extents]
        self.channels = int(channels)
        self.n_frames = int(n_frames)
        self.frame_px = sum(h * w for h, w in self.extents)
        n = self.n_frames * self.frame_px * self.channels
        if is_torch_tensor(data):
            data = data.reshape(-1)
        else:
            data = np.ascontiguousarray(data, dtype=self.dtype).reshape(-1)
        if data.shape[0] != n:
            raise ValueError("PackedPyramid: buffer holds %d floats, extents need %d" % (data.shape[0], n))
        if is_torch_tensor(data) and data.element_size() != self.dtype.itemsize:
            raise ValueError("PackedPyramid: a %s buffer for dtype %s" % (data.dtype, self.dtype))
        self.data = data

    @property
    def on_device(self):
        return is_torch_tensor(self.data)

    @classmethod
    def from_levels(cls, levels):
        """levels: list of [n_frames, h_l, w_l, C] float32 ndarrays."""
        n_frames, c = levels[0].shape[0], levels[0].shape[-1]
        ext = [l.shape[1:3] for l in levels]
        per_frame = [np.concatenate([np.ascontiguousarray(l[f], np.float32).reshape(-1) for l in levels])
                     for f in range(n_frames)]
        return cls(np.concatenate(per_frame), ext, c, n_frames)

    def level(self, l):
        """[n_frames, h_l, w_l, C] view (host: NumPy view; device: torch view)."""
        h, w = self.extents[l]
        off = sum(eh * ew for eh, ew in self.extents[:l]) * self.channels
        n = h * w * self.channels
        return self.data.reshape(self.n_frames, -1)[:, off:off + n].reshape(self.n_frames, h, w, self.channels)

    def levels(self):
        return [self.level(l) for l in range(len(self.extents))]

    def like(self, channels, data=None):
        """Same geometry, other channel count; allocates when data is None."""
        n = self.n_frames * self.frame_px * channels
        if data is None:
            if self.on_device:
                import torch
                data = torch.empty(n, dtype=self.data.dtype, device=self.data.device)
            else:
                data = np.empty(n, dtype=self.dtype)
        return PackedPyramid(data, self.extents, channels, self.n_frames, dtype=self.dtype)


class _Operand(object):
    """Normalised view of an input tensor: geometry + pointer + how to allocate results and which entry point to call.
    ``ctx``: the context to run on (default: the shared one of the tensor's device)."""

    def __init__(self, x, channels=None, ctx=None, frame_dtype="float32", frame_layout="packed"):
        self.packed = isinstance(x, PackedPyramid)
        strided = frame_layout == "strided"      # (uint8 / uint16 frames: checked by the caller) the frames are a view, passed as it is
        narrow = frame_dtype in ("uint8", "uint16")
        if narrow and not strided:
            _require_narrow(x, frame_dtype)
        if self.packed:
            self.src = x
            buf = x.data
            self.extents, self.n_frames, self.c = x.extents, x.n_frames, x.channels
            self.dev = x.on_device
        elif isinstance(x, np.ndarray) or is_torch_tensor(x):
            if x.ndim != 4:
                raise ValueError("expected a rank-4 NHWC tensor, got shape %s" % (tuple(x.shape),))
            n, h, w, c = (int(s) for s in x.shape)
            if min(n, h, w, c) < 1:
                raise ValueError("empty tensor: shape %s" % (tuple(x.shape),))
            self.extents, self.n_frames, self.c = [(h, w)], n, c
            self.dev = is_torch_tensor(x)
            buf = x
        else:
            raise TypeError(TYPE_ERROR_MESSAGE)
        if channels is not None and self.c != channels:
            raise ValueError("tensor has %d channels, expected %d" % (self.c, channels))
        if self.dev:
            import torch
            if not buf.is_cuda:
                raise TypeError("torch tensors must live on the GPU (use a numpy array for host data)")
            if not narrow:
                buf = as_float32(buf)
            self.device = buf.device.index or 0
            self.stream = C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)
            self.ptr = C.c_void_p(buf.data_ptr())
            self._torch_device = buf.device
        else:
            if not strided:
                buf = np.ascontiguousarray(buf, dtype=getattr(np, frame_dtype) if narrow else np.float32)
            self.device = None
            self.stream = None
            self.ptr = C.c_void_p(buf.ctypes.data)
        if strided:
            view = frame_view_of(buf, self.c, frame_dtype)
            self.ptr = _lib.view16_ptr(view) if frame_dtype == "uint16" else _lib.view_ptr(view)
        elif frame_dtype == "uint8":
            self.ptr = _lib.byte_ptr(self.ptr.value)
        elif frame_dtype == "uint16":
            self.ptr = _lib.short_ptr(self.ptr.value)
        self.buf = buf                                  # keep alive
        self.frame_px = sum(h * w for h, w in self.extents)
        self.levels = (_lib.Extent * len(self.extents))(*[_lib.Extent(h, w) for h, w in self.extents])
        self.n_levels = len(self.extents)
        self.ctx = ctx or get_context(self.device)

    def empty(self, shape, dtype=np.float32):
        """A result buffer placed like the operand (torch tensor on its device, or ndarray) and its address."""
        if self.dev:
            import torch
            out = torch.empty(shape, dtype={np.float32: torch.float32, np.int64: torch.int64, np.float16: torch.float16}[dtype],
                              device=self._torch_device)
            return out, C.c_void_p(out.data_ptr())
        out = np.empty(shape, dtype=dtype)
        return out, C.c_void_p(out.ctypes.data)

    def alloc(self, channels):
        return self.empty(self.n_frames * self.frame_px * channels)

    def call(self, name, *args):
        """silent_<name>_dev(ctx, *args, stream) on torch's current stream for a device operand, the synchronous host-pointer
        silent_<name>(ctx, *args) otherwise."""
        if self.dev:
            rc = getattr(_lib.load(), "silent_" + name + "_dev")(self.ctx.handle, *(args + (self.stream,)))
        else:
            rc = getattr(_lib.load(), "silent_" + name)(self.ctx.handle, *args)
        self.ctx.check(rc)

    def wrap(self, flat, channels):
        if self.packed:
            return PackedPyramid(flat, self.extents, channels, self.n_frames)
        h, w = self.extents[0]
        return flat.reshape(self.n_frames, h, w, channels)

    def geom(self):
        return (self.levels, self.n_levels, self.n_frames)


def _require_narrow(x, frame_dtype="uint8"):
    """frame_dtype="uint8" / "uint16": the frames are passed as they are, so they must BE of that type (uint16: in native byte order)
    -- an ndarray, or a contiguous GPU tensor."""
    if isinstance(x, np.ndarray):
        ok = x.dtype == getattr(np, frame_dtype) and x.dtype.isnative
    elif is_torch_tensor(x):
        import torch
        ok = x.dtype == getattr(torch, frame_dtype) and x.is_contiguous()
    else:
        raise TypeError(TYPE_ERROR_MESSAGE)
    if not ok:
        raise ValueError("frame_dtype='%s' takes a %s ndarray or a contiguous %s GPU tensor (nothing is converted), got %s"
                         % (frame_dtype, frame_dtype, frame_dtype, x.dtype))


def _require_uint8(x):
    _require_narrow(x, "uint8")


def frame_view_of(frames, channels, frame_dtype=None):
    """A uint8 array -- torch tensor or ndarray, [n, H, W, channels] with channels 1 or 3, or [n, H, W] for one channel -- as the
    view the silent_*_view entry points read in place: (address, channels, pixel_stride, row_stride, frame_stride), strides in bytes.
    A uint16 array (native byte order; channels 1: [n, H, W] or [n, H, W, 1]) gives the view of the silent_*_view16 entry points in
    the same form, its strides in BYTES as well (even) -- p010[:, :H, :W] of pitched surfaces, rgba16[..., 1], a window of larger
    frames.  frame_dtype: None takes either type, "uint8" / "uint16" only that one.
    Any positive strides do (a pitched surface, bgra[..., :3], yuyv[:, :, ::2, None], a region of a larger frame, every second
    frame); a ValueError for anything but uint8, for a negative or zero stride ([::-1], a broadcast), for strides under which pixels
    or rows overlap, and for three channels that are not adjacent bytes.  An axis of length 1 has no stride to speak of: it is
    given the smallest valid one."""
    if isinstance(channels, bool) or not isinstance(channels, int) or channels not in FRAME_CHANNELS:
        raise ValueError("frame_view_of: channels must be 1 or 3, got %r" % (channels,))
    if frame_dtype not in (None, "uint8", "uint16"):
        raise ValueError("frame_view_of: frame_dtype must be 'uint8' or 'uint16', got %r" % (frame_dtype,))
    if isinstance(frames, np.ndarray):
        wide = frames.dtype == np.uint16 and frames.dtype.isnative
        ok, strides, address = frames.dtype == np.uint8 or wide, tuple(int(s) for s in frames.strides), frames.ctypes.data
    elif is_torch_tensor(frames):
        import torch
        wide = frames.dtype == torch.uint16
        ok, strides, address = frames.dtype == torch.uint8 or wide, tuple(int(s) * (2 if wide else 1) for s in frames.stride()), frames.data_ptr()
    else:
        raise TypeError(TYPE_ERROR_MESSAGE)
    if not ok or (frame_dtype is not None and wide != (frame_dtype == "uint16")):
        raise ValueError("frame_view_of takes %s frames (nothing is converted), got %s"
                         % ("uint8 or uint16" if frame_dtype is None else frame_dtype, frames.dtype))
    if wide:
        return _frame_view16_of(frames, channels, strides, address)
    shape = tuple(int(s) for s in frames.shape)
    if len(shape) == 3 and channels == 1:
        shape, strides = shape + (1,), strides + (1,)
    if len(shape) != 4 or shape[3] != channels:
        raise ValueError("frame_view_of: expected [n, H, W, %d]%s, got shape %s"
                         % (channels, " or [n, H, W]" if channels == 1 else "", tuple(frames.shape)))
    n, h, w, _ = shape
    if min(n, h, w) < 1:
        raise ValueError("frame_view_of: empty frames, shape %s" % (tuple(frames.shape),))
    sn, sh, sw, sc = strides
    if channels == 3 and sc != 1:
        raise ValueError("frame_view_of: the three channels of a pixel must be adjacent bytes (channel stride 1), got %d" % sc)
    for name, length, stride in (("frame", n, sn), ("row", h, sh), ("pixel", w, sw)):
        if length > 1 and stride <= 0:
            raise ValueError("frame_view_of: %s stride %d: a view is never flipped or broadcast (strides must be positive)"
                             % (name, stride))
    pixel = sw if w > 1 else channels
    row_min = (w - 1) * pixel + channels
    row = sh if h > 1 else row_min
    frame_min = (h - 1) * row + row_min
    frame = sn if n > 1 else frame_min
    if pixel < channels or row < row_min or frame < frame_min:
        raise ValueError("frame_view_of: pixels, rows or frames of the view overlap (strides %s for shape %s)" % (strides, shape))
    return int(address), channels, pixel, row, frame


def _frame_view16_of(frames, channels, strides, address):
    """frame_view_of for uint16 frames: one 2-byte element per pixel, `strides` in bytes."""
    if channels != 1:
        raise ValueError("frame_view_of: uint16 frames have one channel, got channels=%r" % (channels,))
    shape = tuple(int(s) for s in frames.shape)
    if len(shape) == 3:
        shape, strides = shape + (1,), strides + (2,)
    if len(shape) != 4 or shape[3] != 1:
        raise ValueError("frame_view_of: expected [n, H, W, 1] or [n, H, W], got shape %s" % (tuple(frames.shape),))
    n, h, w, _ = shape
    if min(n, h, w) < 1:
        raise ValueError("frame_view_of: empty frames, shape %s" % (tuple(frames.shape),))
    sn, sh, sw, _ = strides
    for name, length, stride in (("frame", n, sn), ("row", h, sh), ("pixel", w, sw)):
        if length > 1 and stride <= 0:
            raise ValueError("frame_view_of: %s stride %d: a view is never flipped or broadcast (strides must be positive)"
                             % (name, stride))
    pixel = sw if w > 1 else 2
    row_min = (w - 1) * pixel + 2
    row = sh if h > 1 else row_min
    frame_min = (h - 1) * row + row_min
    frame = sn if n > 1 else frame_min
    if pixel < 2 or row < row_min or frame < frame_min:
        raise ValueError("frame_view_of: pixels, rows or frames of the view overlap (strides %s for shape %s)" % (strides, shape))
    if (address | pixel | row | frame) & 1:
        raise ValueError("frame_view_of: uint16 frames need an even address and even byte strides (strides %s)" % (strides,))
    return int(address), 1, pixel, row, frame


def _kernel_arg(k, c_in=None):
    k = np.ascontiguousarray(np.asarray(k, dtype=np.float64).astype(np.float32))   # tf.constant(k, float32)
    if k.ndim != 4:
        raise ValueError("filter must be HWIO rank 4, got shape %s" % (k.shape,))
    if c_in is not None and k.shape[2] != c_in:
        raise ValueError("filter C_in %d does not match tensor channels %d" % (k.shape[2], c_in))
    return k


def _same_geometry(a, b, what):
    if a.extents != b.extents or a.n_frames != b.n_frames or a.dev != b.dev:
        raise ValueError("%s: tensors differ in geometry or placement" % what)


# ----------------------------------------------------------------------------- op wrappers

def conv2d_same(x, kernel_hwio, relu=False, clip_hi=None):
    op = _Operand(x)
    k = _kernel_arg(kernel_hwio, op.c)
    kh, kw, _, co = k.shape
    out, optr = op.alloc(co)
    flags = (_lib.RELU if relu else 0) | (_lib.CLIP if clip_hi is not None else 0)
    op.call("conv2d_same", op.ptr, *op.geom(), op.c, C.c_void_p(k.ctypes.data), kh, kw, co, flags, float(clip_hi or 0.0), optr)
    return op.wrap(out, co)


def regulate(x, blur_hwio, regulation_value, regulation_root=0.5, flat_policy="ieee"):
    op = _Operand(x)
    k = _kernel_arg(blur_hwio, op.c)
    if k.shape[3] != op.c:
        raise ValueError("blur tensor must be [kh, kw, C, C]")
    try:
        pol = {"ieee": _lib.FLAT_IEEE, "zero": _lib.FLAT_ZERO}[flat_policy]
    except KeyError:
        raise ValueError("flat_policy must be 'ieee' or 'zero'")
    out, optr = op.alloc(op.c)
    op.call("regulate", op.ptr, *op.geom(), op.c, C.c_void_p(k.ctypes.data), k.shape[0], k.shape[1], float(regulation_value),
            float(regulation_root), pol, optr)
    return op.wrap(out, op.c)


def gray_line_end(x, cs_kernel, end_bank, clip_hi=255.0, want_cs=True, want_end=True):
    op = _Operand(x, channels=1)
    cs = _kernel_arg(cs_kernel, 1)
    eb = _kernel_arg(end_bank, 1)
    if cs.shape != (3, 3, 1, 1) or eb.shape[:3] != (3, 3, 1):
        raise ValueError("gray_line_end needs a [3,3,1,1] CS kernel and a [3,3,1,K] end bank")
    K = eb.shape[3]
    cs_out, cs_ptr = op.alloc(1) if want_cs else (None, None)
    end_out, end_ptr = op.alloc(K) if want_end else (None, None)
    op.call("gray_line_end", op.ptr, *op.geom(), C.c_void_p(cs.ctypes.data), C.c_void_p(eb.ctypes.data), K, float(clip_hi), cs_ptr,
            end_ptr)
    return (op.wrap(cs_out, 1) if want_cs else None, op.wrap(end_out, K) if want_end else None)


def pad_inwards(x, pt, pb, pl, pr):
    op = _Operand(x)
    out, optr = op.alloc(op.c)
    op.call("pad_inwards", op.ptr, *op.geom(), op.c, int(pt), int(pb), int(pl), int(pr), optr)
    return op.wrap(out, op.c)


def value_from_color(x):
    op = _Operand(x)
    out, optr = op.alloc(1)
    op.call("value_from_color", op.ptr, *op.geom(), op.c, optr)
    return op.wrap(out, 1)


def bw_from_color(x):
    op = _Operand(x)
    out, optr = op.alloc(1)
    op.call("bw_from_color", op.ptr, *op.geom(), op.c, optr)
    return op.wrap(out, 1)


def nms3x3(x, mode="product"):
    op = _Operand(x)
    try:
        m = {"product": _lib.NMS_PRODUCT, "fired": _lib.NMS_FIRED}[mode]
    except KeyError:
        raise ValueError("mode must be 'product' or 'fired'")
    out, optr = op.alloc(op.c)
    op.call("nms3x3", op.ptr, *op.geom(), op.c, m, optr)
    return op.wrap(out, op.c)


def top_value_points(color, top_percent=0.1, value=None):
    op = _Operand(color)
    vptr = None
    if value is not None:
        vop = _Operand(value, channels=1)
        _same_geometry(op, vop, "top_value_points")
        vptr = vop.ptr
    out, optr = op.alloc(op.c)
    op.call("top_value_points", op.ptr, vptr, *op.geom(), op.c, float(top_percent), optr)
    return op.wrap(out, op.c)


def max_value_indices_region(value, regions, cap_per_frame=None):
    """value: 1-channel tensor.  regions: one (rH, rW) per level.  Returns (idx [n_frames, cap, 4] int64,
    counts [n_frames] int64) -- host arrays for host input, torch tensors for device input."""
    op = _Operand(value, channels=1)
    if len(regions) != op.n_levels:
        raise ValueError("need one (rH, rW) region per level")
    reg = (_lib.Extent * op.n_levels)(*[_lib.Extent(int(rh), int(rw)) for rh, rw in regions])
    cap = op.frame_px if cap_per_frame is None else int(cap_per_frame)
    idx, iptr = op.empty((op.n_frames, cap, 4), np.int64)
    counts, cptr = op.empty(op.n_frames, np.int64)
    op.call("max_value_indices_region", op.ptr, *op.geom(), reg, iptr, cap, cptr)
    return idx, counts


def select_peaks(color, top_percent=0.1, value=None, want=("top", "peaks", "peak_value")):
    """silent_select_peaks: top_value_points -> nms3x3 (product) -> value in one pass.  Returns a dict."""
    op = _Operand(color)
    vptr = None
    if value is not None:
        vop = _Operand(value, channels=1)
        _same_geometry(op, vop, "select_peaks")
        vptr = vop.ptr
    outs, ptrs = {}, {}
    for name, ch in (("top", op.c), ("peaks", op.c), ("peak_value", 1)):
        if name in want:
            outs[name], ptrs[name] = op.alloc(ch)
        else:
            ptrs[name] = None
    op.call("select_peaks", op.ptr, vptr, *op.geom(), op.c, float(top_percent), ptrs["top"], ptrs["peaks"], ptrs["peak_value"])
    return {n: op.wrap(o, 1 if n == "peak_value" else op.c) for n, o in outs.items()}


def centroids(value, region_h, region_w):
    """silent_centroids: (L1 distance map like ``value``, total_pool as a tensor of cells)."""
    op = _Operand(value, channels=1)
    rh, rw = int(region_h), int(region_w)
    if rh < 1 or rw < 1:
        raise ValueError("region extents must be >= 1")
    cell_ext = [(-(-h // rh), -(-w // rw)) for h, w in op.extents]
    n_cells = op.n_frames * sum(a * b for a, b in cell_ext)
    dist, dptr = op.alloc(1)
    tot, tptr = op.empty(n_cells)
    op.call("centroids", op.ptr, *op.geom(), rh, rw, dptr, tptr)
    if op.packed:
        return op.wrap(dist, 1), PackedPyramid(tot, cell_ext, 1, op.n_frames)
    return op.wrap(dist, 1), tot.reshape(op.n_frames, cell_ext[0][0], cell_ext[0][1], 1)


def _require_inplace(state):
    """The boosting state is updated in place: it has to be float32 and contiguous already (no hidden copy)."""
    data = state.data if isinstance(state, PackedPyramid) else state
    if isinstance(data, np.ndarray):
        ok = data.dtype == np.float32 and data.flags["C_CONTIGUOUS"] and data.flags["WRITEABLE"]
    elif is_torch_tensor(data):
        import torch
        ok = data.dtype == torch.float32 and data.is_contiguous()
    else:
        raise TypeError(TYPE_ERROR_MESSAGE)
    if not ok:
        raise ValueError("the boosting state must be a writable, contiguous float32 tensor (it is updated in place)")


def boosting_step(x, energy, exhaustion_max=1.0, excitation_max=1.0, recovery_mode=_lib.RECOVERY_CONSTANT,
                  visualize=False, recovery_amount=10.0, recovery_percentage=0.8):
    """silent_boosting_step: advances ``energy`` in place, returns (fired map, energy map) -- 3 channels each when
    ``visualize``."""
    _require_inplace(energy)
    op, st = _Operand(x, channels=1), _Operand(energy, channels=1)
    _same_geometry(op, st, "boosting_step")
    c = 3 if visualize else 1
    fired, fptr = op.alloc(c)
    eout, eptr = op.alloc(c)
    params = _lib.BoostingParams(float(exhaustion_max), float(excitation_max), int(recovery_mode),
                                 float(recovery_amount), float(recovery_percentage), 1 if visualize else 0)
    op.call("boosting_step", op.ptr, *op.geom(), C.byref(params), st.ptr, fptr, eptr)
    return op.wrap(fired, c), op.wrap(eout, c)


ATTENTION_RESIZE_DIV = float(np.float32(float(np.e) ** .5))      # recognition_testing.py:82-83: float32(e ** .5)


def attention_params(region=(3, 3), resize_div=None, exhaustion_max=1.0, excitation_max=1.0, recovery_mode=_lib.RECOVERY_CONSTANT,
                     visualize=True, recovery_amount=10.0, recovery_percentage=0.8):
    """A silent_attention_params: the centroid region, the divisor of the half map and the boosting parameters."""
    rh, rw = (int(v) for v in region)
    if rh < 1 or rw < 1:
        raise ValueError("region extents must be >= 1")
    return _lib.AttentionParams(rh, rw, ATTENTION_RESIZE_DIV if resize_div is None else float(resize_div),
                                _lib.BoostingParams(float(exhaustion_max), float(excitation_max), int(recovery_mode), float(recovery_amount),
                                                    float(recovery_percentage), 1 if visualize else 0))


def attention_extents(extents, params):
    """silent_attention_extents (host only, no GPU work): per level the cell extents of the map, the half extents and the cell extents
    of the half map, as three lists of (h, w).  ValueError for what silent_attention_tail refuses of the geometry."""
    n = len(extents)
    levels = (_lib.Extent * max(n, 1))(*[_lib.Extent(int(h), int(w)) for h, w in extents])
    out = [(_lib.Extent * max(n, 1))() for _ in range(3)]
    _lib.check(_lib.load().silent_attention_extents(levels, n, C.byref(params), *out))
    return tuple([(int(e.h), int(e.w)) for e in o[:n]] for o in out)


def attention_tail(value, energy, region=(3, 3), resize_div=None, exhaustion_max=1.0, excitation_max=1.0,
                   recovery_mode=_lib.RECOVERY_CONSTANT, visualize=True, recovery_amount=10.0, recovery_percentage=0.8,
                   want=("centroids", "centroids2", "fired", "update")):
    """silent_attention_tail: what LineEndDisplayer.compile computes after the line-end map (recognition_testing.py:77-100) on a batch
    of 1-channel value maps -- a PackedPyramid or an NHWC tensor, every frame a stream of its own -- in two launches.  ``energy``: the
    boosting state, one value per centroid cell (a PackedPyramid with the cell extents / a tensor [n, ceil(h / rh), ceil(w / rw), 1]),
    advanced in place.  Returns (255 - centroids * 255, the same on the nearest-neighbour half map, fired * 255, update_importances) as
    PackedPyramids / tensors like ``value``; fired and update have 3 channels when ``visualize``.  ``want``: the results to compute
    (None in the place of the others; without "centroids2" nothing of the half map is computed)."""
    unknown = set(want) - {"centroids", "centroids2", "fired", "update"}
    if unknown:
        raise ValueError("attention_tail: unknown result %s" % sorted(unknown))
    _require_inplace(energy)
    op, st = _Operand(value, channels=1), _Operand(energy, channels=1)
    params = attention_params(region, resize_div, exhaustion_max, excitation_max, recovery_mode, visualize, recovery_amount, recovery_percentage)
    cells, half, _ = attention_extents(op.extents, params)
    if st.extents != cells or st.n_frames != op.n_frames or st.dev != op.dev:
        raise ValueError("attention_tail: the state must hold one value per centroid cell, %s per frame, placed like the value map" % (cells,))
    c = 3 if visualize else 1
    n_cells = op.n_frames * sum(h * w for h, w in cells)
    sizes = {"centroids": op.n_frames * op.frame_px, "centroids2": op.n_frames * sum(h * w for h, w in half), "fired": n_cells * c,
             "update": n_cells * c}
    bufs = {k: op.empty(sizes[k]) if k in want else (None, None) for k in ("centroids", "centroids2", "fired", "update")}
    op.call("attention_tail", op.ptr, *op.geom(), C.byref(params), st.ptr, *[bufs[k][1] for k in ("centroids", "centroids2", "fired", "update")])

    def wrap(k, ext, ch):
        if bufs[k][0] is None:
            return None
        if op.packed:
            return PackedPyramid(bufs[k][0], ext, ch, op.n_frames)
        return bufs[k][0].reshape(op.n_frames, ext[0][0], ext[0][1], ch)
    return wrap("centroids", op.extents, 1), wrap("centroids2", half, 1), wrap("fired", cells, c), wrap("update", cells, c)


def affine_clip(x, mul=1.0, add=0.0, lo=-float("inf"), hi=float("inf"), post_add=0.0, div=1.0):
    """silent_affine_clip: clip(x * mul / div + add, lo, hi) + post_add, any channel count."""
    op = _Operand(x)
    out, optr = op.alloc(op.c)
    params = _lib.AffineParams(float(mul), float(div), float(add), float(lo), float(hi), float(post_add))
    op.call("affine_clip", op.ptr, op.n_frames * op.frame_px * op.c, C.byref(params), optr)
    return op.wrap(out, op.c)


def gather_to_host(tensors):
    """Contiguous float32 GPU tensors (torch) -> one flat float32 np.ndarray holding them back to back
    (silent_gather_d2h: n async device-to-host copies on the tensors' current stream, ONE synchronisation)."""
    import torch
    n = len(tensors)
    if n == 0:
        return np.empty(0, np.float32)
    dev = tensors[0].device
    for t in tensors:
        if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("gather_to_host: contiguous float32 tensors on one GPU expected")
    ctx = get_context(dev.index)
    host = np.empty(sum(t.numel() for t in tensors), np.float32)
    srcs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    sizes = (C.c_size_t * n)(*[t.numel() * 4 for t in tensors])
    ctx.check(ctx._lib.silent_gather_d2h(ctx.handle, C.c_void_p(host.ctypes.data), srcs, sizes, n,
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return host


def resize_nearest(x, out_extents):
    """silent_resize_nearest.  ``out_extents``: one (h, w) for an NHWC tensor, one per level for a PackedPyramid."""
    op = _Operand(x)
    if not op.packed:
        out_extents = [tuple(out_extents)] if np.ndim(out_extents[0]) == 0 else list(out_extents)
    out_extents = [(int(h), int(w)) for h, w in out_extents]
    if len(out_extents) != op.n_levels or min(min(e) for e in out_extents) < 1:
        raise ValueError("resize_nearest: need one positive (h, w) per level")
    out_levels = (_lib.Extent * op.n_levels)(*[_lib.Extent(h, w) for h, w in out_extents])
    out, optr = op.empty(op.n_frames * sum(h * w for h, w in out_extents) * op.c)
    op.call("resize_nearest", op.ptr, *op.geom(), op.c, out_levels, optr)
    if op.packed:
        return PackedPyramid(out, out_extents, op.c, op.n_frames)
    return out.reshape(op.n_frames, out_extents[0][0], out_extents[0][1], op.c)


def rgb_line_end(x, kernels, regulation_value=1.0, regulation_root=0.1, flat_policy="ieee", clip_hi=255.0, pad=2,
                 want=("orient", "line_end", "value"), storage="float32"):
    """The reference graph recognition_testing.py:69-77 on 3-channel levels.  ``kernels``: dict with
    rgc, rgby, stripe, end ([3,3,3,3]) and blur ([7,7,3,3]).  Returns dict of the requested outputs.  ``storage="float16"``:
    orient and line_end come back as float16 maps (silent_rgb_line_end_h: the float32 results rounded once at the store)."""
    if storage not in STORAGES:
        raise ValueError("storage must be 'float32' or 'float16', got %r" % (storage,))
    half = storage == "float16"
    op = _Operand(x, channels=3)
    ks = {}
    for name, shape in (("rgc", (3, 3, 3, 3)), ("rgby", (3, 3, 3, 3)), ("stripe", (3, 3, 3, 3)),
                        ("blur", (7, 7, 3, 3)), ("end", (3, 3, 3, 3))):
        k = _kernel_arg(kernels[name], 3)
        if k.shape != shape:
            raise ValueError("kernel %s must have shape %s, got %s" % (name, shape, k.shape))
        ks[name] = k
    fp = C.POINTER(C.c_float)
    params = _lib.RgbChainParams(*[ks[n].ctypes.data_as(fp) for n in ("rgc", "rgby", "stripe", "blur", "end")],
                                 float(regulation_value), float(regulation_root),
                                 {"ieee": _lib.FLAT_IEEE, "zero": _lib.FLAT_ZERO}[flat_policy], float(clip_hi), int(pad))
    outs, ptrs = {}, {}
    for name, ch in (("orient", 3), ("line_end", 3), ("value", 1)):
        if name in want and half and ch == 3:
            outs[name], ptrs[name] = op.empty(op.n_frames * op.frame_px * ch, np.float16)
            ptrs[name] = _lib.half_ptr(ptrs[name].value)
        elif name in want:
            outs[name], ptrs[name] = op.alloc(ch)
        else:
            ptrs[name] = None
    op.call("rgb_line_end_h" if half else "rgb_line_end", op.ptr, *op.geom(), C.byref(params), ptrs["orient"], ptrs["line_end"], ptrs["value"])

    def wrap(n, o):
        if half and n != "value":
            return PackedPyramid(o, op.extents, 3, op.n_frames, dtype=np.float16) if op.packed else o.reshape(op.n_frames, *op.extents[0], 3)
        return op.wrap(o, 1 if n == "value" else 3)
    return {n: wrap(n, o) for n, o in outs.items()}


# ----------------------------------------------------------------------------- pyramid plans

class FrameDisplayer(object):
    """silent_displayer: one camera frame -> the six fetched tensors of the reference's graph, ONE library call per frame
    (recognition_testing.py:106-144 as a replayed HIP graph; include/silent_hip.h).  ``frame_shape`` (H, W, 3), ``dtype`` the
    frames' NumPy dtype, ``output_size`` (w, h) and ``zoom_ratio`` as PyramidDisplayer takes them."""

    _DT = {"uint8": _lib.DT_U8, "float32": _lib.DT_F32, "float64": _lib.DT_F64, "int32": _lib.DT_I32, "uint16": _lib.DT_U16,
           "int16": _lib.DT_I16, "int64": _lib.DT_I64}

    def __init__(self, frame_shape, dtype, output_size, zoom_ratio, kernels, centroid_region=(3, 3), recovery_mode=_lib.RECOVERY_CONSTANT,
                 flat_policy="ieee", clip_hi=255.0, pad=2, device=None):
        from .util.zoom.from_image import reference_levels
        h, w, c = (int(v) for v in frame_shape)
        if c != 3:
            raise ValueError("FrameDisplayer takes [H, W, 3] frames")
        self.dtype = np.dtype(dtype)
        if self.dtype.name not in self._DT:
            raise TypeError("frames of dtype %s are not supported" % self.dtype)
        self.frame_shape = (h, w, 3)
        self.ctx = get_context(device)
        levels = reference_levels((h, w), output_size, zoom_ratio)
        if not levels:
            raise ValueError("the frame is not larger than output_size: image_to_zoom_tensor has no level (from_image.py:45-46)")
        arr = (_lib.PyrLevel * len(levels))(*[_lib.PyrLevel(*[int(v) for v in l]) for l in levels])
        self._kernels = {k: np.ascontiguousarray(kernels[k], np.float32) for k in ("rgc", "rgby", "stripe", "blur", "end")}
        fp = C.POINTER(C.c_float)
        chain = _lib.RgbChainParams(*[self._kernels[k].ctypes.data_as(fp) for k in ("rgc", "rgby", "stripe", "blur", "end")],
                                    1.0, 0.1, {"ieee": _lib.FLAT_IEEE, "zero": _lib.FLAT_ZERO}[flat_policy], float(clip_hi), int(pad))
        boost = _lib.BoostingParams(1.0, 1.0, int(recovery_mode), 10.0, 0.8, 1)
        prm = _lib.DisplayerParams(h, w, self._DT[self.dtype.name], int(centroid_region[0]), int(centroid_region[1]), chain, boost)
        self.handle = C.c_void_p()
        lib = self._lib = _lib.load()
        self.ctx.check(lib.silent_displayer_create(self.ctx.handle, C.byref(prm), arr, len(levels), C.byref(self.handle)))
        shape, floats = (C.c_int32 * 7)(), (C.c_size_t * 6)()
        self.ctx.check(lib.silent_displayer_shape(self.handle, shape, floats))
        L, lh, lw, ch, cw, hh, hw = (int(v) for v in shape)
        self.shapes = [(L, lh, lw, 3), (L, lh, lw, 1), (L, hh, hw, 1), (L, ch, cw, 3), (L, ch, cw, 3), (L, lh, lw, 3)]
        self.state_shape = (L, ch, cw, 1)
        assert [int(np.prod(sh)) for sh in self.shapes] == [int(f) for f in floats]
        self._res = (C.c_void_p * 6)()
        self._ms = C.c_float(0)
        self.gpu_ms = 0.0
        self._exports = []                  # weak references to the ctypes buffers handed out as views (frame_buffer, step results)
        ptr, nbytes = C.c_void_p(), C.c_size_t(0)
        self.ctx.check(lib.silent_displayer_input(self.handle, C.byref(ptr), C.byref(nbytes)))
        buf = (C.c_char * nbytes.value).from_address(ptr.value)
        buf._owner = self
        self._exports.append(weakref.ref(buf))
        #: the displayer's pinned input buffer as an [H, W, 3] array: a capture loop that grabs INTO it (``cap.read(disp.frame_buffer)``,
        #: ``np.copyto``) and passes it to ``step`` is uploaded without the staging copy
        self.frame_buffer = np.frombuffer(buf, self.dtype).reshape(self.frame_shape)

    #: result slots a displayer may hold for ``step(hold=True)`` before it falls back to copying (3.55 MB each at 640 x 480)
    MAX_HELD_SLOTS = 8

    def step(self, frame, copy=False, timing=False, hold=False):
        """frame: [H, W, 3] ndarray of the displayer's dtype.  Returns the six float32 arrays, in one of three ways:

        ``hold=True`` -- what ``LineEndDisplayer.callback`` hands out: arrays that stay valid FOR AS LONG AS THEY ARE REFERENCED, like the
        fresh arrays of the reference's session.run (recognition_testing.py:132), without a copy: the frame is stepped into a pinned
        result slot nobody references any more (the displayer keeps weak references to what it handed out; slots are added on demand,
        at most MAX_HELD_SLOTS); when every slot is still held the frame goes through the two alternating slots and is COPIED out.
        ``copy=False`` (default) -- the raw form: views of one of two alternating slots, valid until the second next raw step.
        ``copy=True`` -- fresh arrays by one memcpy of the slot.
        All views (and ``frame_buffer``) keep the displayer alive; ``close`` defers the free while they exist.
        ``timing``: also measure the device time of the frame (``gpu_ms``; HIP events around the graph and a stream synchronisation
        instead of the poll of the frame's completion word: ~0.02 ms more wall time)."""
        if not getattr(self, "handle", None):
            raise RuntimeError("the displayer is closed")
        if not isinstance(frame, np.ndarray) or frame.dtype != self.dtype or tuple(frame.shape) != self.frame_shape:
            raise ValueError("frame must be a %s ndarray of shape %s" % (self.dtype, self.frame_shape,))
        f = frame if frame.flags["C_CONTIGUOUS"] else np.ascontiguousarray(frame)
        ms = C.byref(self._ms) if timing else None
        slot = None
        if hold:
            slot = self._free_slot()
            if slot is None:
                copy = True                     # every slot is still referenced by somebody: this frame is copied out
        if slot is None:
            self.ctx.check(self._lib.silent_displayer_step(self.handle, C.c_void_p(f.ctypes.data), self._res, ms))
        else:
            self.ctx.check(self._lib.silent_displayer_step_slot(self.handle, C.c_void_p(f.ctypes.data), slot, self._res, ms))
        if timing:
            self.gpu_ms = float(self._ms.value)
        out = []
        if copy and slot is None:
            # ONE copy of the whole slot (the six results lie back to back, 64-byte steps), then views of the copy
            ptrs = [int(p) for p in self._res]
            total = (max(ptrs) - min(ptrs)) // 4 + int(np.prod(self.shapes[ptrs.index(max(ptrs))]))
            whole = np.frombuffer((C.c_float * total).from_address(min(ptrs)), np.float32).copy()
            for ptr, sh in zip(ptrs, self.shapes):
                o = (ptr - min(ptrs)) // 4
                out.append(whole[o:o + int(np.prod(sh))].reshape(sh))
            return out
        refs = self._exports if slot is None else self._held[slot]
        for ptr, sh in zip(self._res, self.shapes):
            buf = (C.c_float * int(np.prod(sh))).from_address(ptr)
            buf._owner = self               # the views keep the displayer (and with it the pinned slot) alive
            refs.append(weakref.ref(buf))
            out.append(np.frombuffer(buf, np.float32).reshape(sh))
        if len(self._exports) > 64:
            self._exports = [r for r in self._exports if r() is not None]
        return out

    def _free_slot(self):
        """A held-results slot (numbers 2, 3, ...: 0 and 1 are the raw alternating pair) nobody references any more; a new one while
        fewer than MAX_HELD_SLOTS exist; None when all are taken."""
        held = self.__dict__.setdefault("_held", {})
        for slot, refs in held.items():
            if not any(r() is not None for r in refs):
                del refs[:]
                return slot
        if len(held) >= self.MAX_HELD_SLOTS:
            return None
        idx = C.c_int(-1)
        self.ctx.check(self._lib.silent_displayer_add_slot(self.handle, C.byref(idx)))
        held[int(idx.value)] = []
        return int(idx.value)

    def get_state(self):
        st = np.empty(self.state_shape, np.float32)
        self.ctx.check(self._lib.silent_displayer_get_state(self.handle, C.c_void_p(st.ctypes.data)))
        return st

    def set_state(self, state):
        st = np.ascontiguousarray(state, np.float32)
        if tuple(st.shape) != self.state_shape:
            raise ValueError("state shape %s does not match the compiled pyramid %s" % (st.shape, self.state_shape))
        self.ctx.check(self._lib.silent_displayer_set_state(self.handle, C.c_void_p(st.ctypes.data)))

    def close(self):
        """Free the displayer (graphs, device buffers, the pinned frame buffer and result slots).  While views handed out by
        ``step(copy=False)`` or ``frame_buffer`` are still referenced the free is DEFERRED: every view keeps the displayer alive
        (``_owner``), and it is destroyed when the last of them goes -- never under an array somebody still holds.  Further
        ``step`` calls raise either way."""
        if not getattr(self, "handle", None):
            return
        fb = self.__dict__.pop("frame_buffer", None)      # our own reference to the input view does not count
        del fb
        live = list(getattr(self, "_exports", ())) + [r for refs in getattr(self, "_held", {}).values() for r in refs]
        if any(r() is not None for r in live):
            self._deferred, self.handle = self.handle, C.c_void_p()
            return
        self._lib.silent_displayer_destroy(self.handle)
        self.handle = C.c_void_p()

    def __del__(self):
        try:
            h = getattr(self, "_deferred", None) or getattr(self, "handle", None)
            if h:                           # nobody references the displayer any more, hence no view either
                self._lib.silent_displayer_destroy(h)
                self.handle = self._deferred = C.c_void_p()
        except Exception:
            pass


ACCUMULATIONS = ("float32", "float64")


def check_accumulation(accumulation):
    """The accumulation argument of PyramidPlan / LineEndPipeline: "float32" (default) or "float64"."""
    if accumulation not in ACCUMULATIONS:
        raise ValueError("accumulation must be 'float32' or 'float64', got %r" % (accumulation,))
    return accumulation


STORAGES = ("float32", "float16")


def check_storage(storage, mode="gray", accumulation="float32", keypoints=False):
    """The storage argument of PyramidPlan.gray_pass / LineEndPipeline: "float32" (default) or "float16" (the CS and end maps of
    the gray pass stored as IEEE binary16, silent_gray_pass_h).  The name is checked first; then the combinations float16 storage
    does not exist for: mode "rgb", accumulation="float64", keypoints=True (the keypoint tail reads the end map as float32)."""
    if storage not in STORAGES:
        raise ValueError("storage must be 'float32' or 'float16', got %r" % (storage,))
    if storage == "float16":
        if mode != "gray":
            raise ValueError("storage='float16' is for mode 'gray' (the RGB maps are stored as float32)")
        if accumulation == "float64":
            raise ValueError("storage='float16' does not combine with accumulation='float64'")
        if keypoints:
            raise ValueError("storage='float16' does not combine with keypoints=True (the keypoint tail reads the end map as float32)")
    return storage


def check_rgb_storage(rgb_storage, mode="rgb", keep_selection_maps=False):
    """The rgb_storage argument of LineEndPipeline: "float32" (default) or "float16" (the orient and line_end maps of the RGB chain
    stored as IEEE binary16, silent_rgb_line_end_h / silent_rgb_keypoints_h).  The name is checked first; then mode "gray" (its
    float16 option is storage="float16") and keep_selection_maps=True (the top / peaks maps come from the float32 per-op kernels)."""
    if rgb_storage not in STORAGES:
        raise ValueError("rgb_storage must be 'float32' or 'float16', got %r" % (rgb_storage,))
    if rgb_storage == "float16":
        if mode != "rgb":
            raise ValueError("rgb_storage='float16' is for mode 'rgb' (the gray pass takes storage='float16')")
        if keep_selection_maps:
            raise ValueError("rgb_storage='float16' does not combine with keep_selection_maps=True (the top / peaks maps come from the float32 per-op kernels)")
    return rgb_storage


FRAME_DTYPES = ("float32", "uint8", "uint16")


def check_frame_dtype(frame_dtype, mode="gray", accumulation="float32"):
    """The frame_dtype argument of PyramidPlan.run / gray_pass / gray_keypoints and LineEndPipeline: "float32" (default: whatever
    comes is widened to float32 first) or "uint8" (uint8 frames read as they are by the silent_*_u8 entry points -- no widening cast,
    no float32 copy of the batch; bit-identical results) or "uint16" (the same for unsigned 16-bit frames in native byte order, the
    silent_*_u16 entry points: Mono10 / 12 / 16, Y16, the luma of P010 -- the value is (float)v, no shift and no scale).  The name is
    checked first; then the combinations uint8 / uint16 frames do not exist for: mode "rgb" and accumulation="float64"."""
    if frame_dtype not in FRAME_DTYPES:
        raise ValueError("frame_dtype must be 'float32' or 'uint8' or 'uint16', got %r" % (frame_dtype,))
    if frame_dtype != "float32":
        if mode != "gray":
            raise ValueError("frame_dtype='%s' is for mode 'gray' (the RGB kernels read float32 frames)" % frame_dtype)
        if accumulation == "float64":
            raise ValueError("frame_dtype='%s' does not combine with accumulation='float64'" % frame_dtype)
    return frame_dtype


FRAME_CHANNELS = (1, 3)


def check_frame_channels(frame_channels, mode="gray", frame_dtype="float32", accumulation="float32"):
    """The frame_channels argument of PyramidPlan.run / gray_pass / gray_keypoints and LineEndPipeline: 1 (default: the frames have
    the channels of the plan / mode) or 3 (interleaved colour uint8 frames [n, H, W, 3] read as they are by the silent_*_u8x3 entry
    points: each pixel enters as (b0 + b1 + b2) * float32(1/3), the reference's get_value_from_color, formed at the load -- no cast
    launch, no value launch, no float32 copy of the batch).  The value is checked first (an int 1 or 3: "3", 3.0 and True are not);
    then what 3 needs: mode "gray", frame_dtype="uint8" and float32 accumulation."""
    if isinstance(frame_channels, bool) or not isinstance(frame_channels, int) or frame_channels not in FRAME_CHANNELS:
        raise ValueError("frame_channels must be 1 or 3, got %r" % (frame_channels,))
    if frame_channels == 3:
        if mode != "gray":
            raise ValueError("frame_channels=3 is for mode 'gray' (mode 'rgb' reads float32 colour frames as colour)")
        if frame_dtype != "uint8":
            raise ValueError("frame_channels=3 needs frame_dtype='uint8' (interleaved colour frames are read as uint8 only)")
        if accumulation == "float64":
            raise ValueError("frame_channels=3 does not combine with accumulation='float64'")
    return frame_channels


FRAME_LAYOUTS = ("packed", "strided")


def check_frame_layout(frame_layout, mode="gray", frame_dtype="float32", accumulation="float32"):
    """The frame_layout argument of PyramidPlan.run / gray_pass / gray_keypoints and LineEndPipeline: "packed" (default: contiguous
    [n, H, W] or [n, H, W, 3] frames) or "strided" (any uint8 or uint16 view with positive strides -- a pitched decoder surface, BGRA, YUYV
    luma, a region of a larger frame -- read in place by the silent_*_view entry points: no packing launch, no second copy of the
    batch; bit-identical to the packed path on the compacted pixels).  The name is checked first; then what "strided" needs: mode
    "gray", frame_dtype="uint8" or "uint16" and float32 accumulation."""
    if frame_layout not in FRAME_LAYOUTS:
        raise ValueError("frame_layout must be 'packed' or 'strided', got %r" % (frame_layout,))
    if frame_layout == "strided":
        if mode != "gray":
            raise ValueError("frame_layout='strided' is for mode 'gray' (the RGB kernels read packed float32 frames)")
        if frame_dtype not in ("uint8", "uint16"):
            raise ValueError("frame_layout='strided' needs frame_dtype='uint8' or 'uint16' (float32 frames are read packed only)")
        if accumulation == "float64":
            raise ValueError("frame_layout='strided' does not combine with accumulation='float64'")
    return frame_layout


RGB_FRAME_DTYPES = ("float32", "uint8")


def check_rgb_frame_dtype(rgb_frame_dtype, mode="rgb", frame_dtype="float32", frame_channels=1, frame_layout="packed"):
    """The rgb_frame_dtype argument of PyramidPlan.run and LineEndPipeline: "float32" (default: nothing changes) or "uint8" (mode
    "rgb" / a 3-channel plan: packed interleaved uint8 colour frames [n, H, W, 3] read as they are by silent_pyramid_rgb8 -- byte c of
    a pixel enters as (float)byte at the load, no cast launch, no float32 copy of the batch; the pyramid is that of
    frames.astype(float32) bit for bit).  A keyword of its own because frame_dtype="uint8" means single-channel frames and stays
    refused for mode "rgb".  The name is checked first; then what "uint8" needs: mode "rgb" and the defaults of frame_dtype,
    frame_channels and frame_layout (those three describe the frames of a gray pass)."""
    if not isinstance(rgb_frame_dtype, str) or rgb_frame_dtype not in RGB_FRAME_DTYPES:
        raise ValueError("rgb_frame_dtype must be 'float32' or 'uint8', got %r" % (rgb_frame_dtype,))
    if rgb_frame_dtype == "uint8":
        if mode != "rgb":
            raise ValueError("rgb_frame_dtype='uint8' is for mode 'rgb' (mode 'gray' takes uint8 frames through frame_dtype)")
        if frame_dtype != "float32":
            raise ValueError("rgb_frame_dtype='uint8' does not combine with frame_dtype=%r (frame_dtype describes the frames of mode 'gray')"
                             % (frame_dtype,))
        if frame_channels != 1:
            raise ValueError("rgb_frame_dtype='uint8' does not combine with frame_channels=%r (the frames are [n, H, W, 3] already)"
                             % (frame_channels,))
        if frame_layout != "packed":
            raise ValueError("rgb_frame_dtype='uint8' does not combine with frame_layout=%r (packed frames only)" % (frame_layout,))
    return rgb_frame_dtype


RGB_FRAME_LAYOUTS = ("packed", "strided")


def check_rgb_frame_layout(rgb_frame_layout, mode="rgb", rgb_frame_dtype="float32", frame_dtype="float32", frame_channels=1,
                           frame_layout="packed"):
    """The rgb_frame_layout argument of PyramidPlan.run and LineEndPipeline: "packed" (default: nothing changes) or "strided" (mode
    "rgb" / a 3-channel plan with rgb_frame_dtype="uint8": ANY uint8 view [n, H, W, 3] with positive strides and channel stride 1 --
    bgra[..., :3], a pitched BGR surface, a region of larger frames -- read in place by silent_pyramid_rgb8_view: no packing launch, no
    second copy of the batch; the pyramid is that of the packed uint8 path on view.contiguous() bit for bit).  A keyword of its own,
    like rgb_frame_dtype: frame_layout describes the frames of mode "gray".  The name is checked first; then what "strided" needs:
    mode "rgb", rgb_frame_dtype="uint8" and the defaults of frame_dtype, frame_channels and frame_layout."""
    if not isinstance(rgb_frame_layout, str) or rgb_frame_layout not in RGB_FRAME_LAYOUTS:
        raise ValueError("rgb_frame_layout must be 'packed' or 'strided', got %r" % (rgb_frame_layout,))
    if rgb_frame_layout == "strided":
        if mode != "rgb":
            raise ValueError("rgb_frame_layout='strided' is for mode 'rgb' (mode 'gray' takes strided frames through frame_layout)")
        if rgb_frame_dtype != "uint8":
            raise ValueError("rgb_frame_layout='strided' needs rgb_frame_dtype='uint8' (float32 colour frames are read packed only)")
        if frame_dtype != "float32":
            raise ValueError("rgb_frame_layout='strided' does not combine with frame_dtype=%r (frame_dtype describes the frames of mode 'gray')"
                             % (frame_dtype,))
        if frame_channels != 1:
            raise ValueError("rgb_frame_layout='strided' does not combine with frame_channels=%r (the frames are [n, H, W, 3] already)"
                             % (frame_channels,))
        if frame_layout != "packed":
            raise ValueError("rgb_frame_layout='strided' does not combine with frame_layout=%r (frame_layout describes the frames of mode 'gray')"
                             % (frame_layout,))
    return rgb_frame_layout


RGB_FRAME_FORMATS = ("interleaved", "nv12", "p010", "p012", "p016")
# and the formats that take a (y, u, v) triple: rgb_frame_format -> chroma shifts (x, y)
YUV_SHIFTS = {"yuv420": (1, 1), "yuv422": (1, 0), "yuv444": (0, 0)}
# and the formats that take a (y, u, v) triple of UINT16 views: rgb_frame_format -> (sx, sy, depth, shift).  "yuv4xxp10" / "p12": the
# code in the LOW bits (FFmpeg's yuv4xxp10le / p12le, I010 ...), "...msb": in the HIGH bits (P210 / P410 / Y210), "p16": all 16 bits
YUV16_FORMATS = dict(("yuv%sp%d%s" % (x, d, a), (sx, sy, d, 16 - d if a else 0))
                     for x, (sx, sy) in (("420", (1, 1)), ("422", (1, 0)), ("444", (0, 0)))
                     for d, a in ((10, ""), (12, ""), (10, "msb"), (12, "msb"), (16, "")))
# and the formats that take ONE uint8 view [n, H, W] of a raw Bayer mosaic: rgb_frame_format -> pattern of silent_bayer_frames (the
# top-left 2 x 2 cell of the VIEW: red at (pattern >> 1, pattern & 1))
BAYER_FORMATS = {"bayer_rggb": 0, "bayer_grbg": 1, "bayer_gbrg": 2, "bayer_bggr": 3}
NV12_MATRICES = {"bt601": (.299, .114), "bt709": (.2126, .0722)}      # (Kr, Kb)
NV12_RANGES = ("limited", "full")
NV12_ORDERS = ("bgr", "rgb")
P010_DEPTHS = {"p010": 10, "p012": 12, "p016": 16}                   # rgb_frame_format -> bits of a code value (shift = 16 - depth)
P010_MATRICES = dict(NV12_MATRICES, bt2020=(.2627, .0593))           # Rec. 2020 defines 10- and 12-bit video only


def check_rgb_frame_format(rgb_frame_format, mode="rgb", rgb_frame_dtype="float32", rgb_frame_layout="packed", frame_dtype="float32",
                           frame_channels=1, frame_layout="packed", hw=None):
    """The rgb_frame_format argument of PyramidPlan.run and LineEndPipeline: "interleaved" (default: nothing changes), "nv12" (mode
    "rgb" / a 3-channel plan: the frames are a pair (y, uv) of uint8 planes as a hardware video decoder emits them -- luma [n, H, W],
    interleaved chroma [n, H / 2, W / 2, 2], both pitched -- read in place by silent_pyramid_nv12 and converted to three float32
    channels in registers: no conversion launch, no copy of the batch; the pyramid is that of the float32 path on the converted
    frames bit for bit) or "p010" / "p012" / "p016" (the same pair as uint16 planes, the 10 / 12 / 16-bit code in the high bits of
    each element: silent_pyramid_p010) or "yuv420" / "yuv422" / "yuv444" (a triple (y, u, v) of uint8 views of ANY positive strides --
    planar I420 / YV12 / I422 / I444, semi-planar NV12 / NV21 / NV16, packed YUYV / UYVY / VUYA: the layout lives in the strides, the
    name gives the chroma subsampling -- read in place by silent_pyramid_yuv) or one of YUV16_FORMATS, "yuv420p10" ... "yuv444p16" (the
    same triple as UINT16 views, read in place by silent_pyramid_yuv16: "yuvXp10" / "yuvXp12" with the code in the low bits, FFmpeg's
    yuvXp10le / yuvXp12le; "yuvXp10msb" / "yuvXp12msb" with the code in the high bits, P210 / P410 / Y210; "yuvXp16").  The name is checked first; then the mode; then that the format is not combined with
    rgb_frame_dtype="uint8", rgb_frame_layout="strided" or the gray frame_* keywords; then that H and W (hw, when given) are even ("yuv422": W; "yuv444": nothing).
    One of BAYER_FORMATS, "bayer_rggb" / "bayer_grbg" / "bayer_gbrg" / "bayer_bggr": the frames are ONE uint8 view [n, H, W] of a raw
    Bayer mosaic (any positive strides), read in place by silent_pyramid_bayer and demosaiced in registers; the same refusals, and H
    and W of at least 2 (odd extents are fine)."""
    if not isinstance(rgb_frame_format, str) or rgb_frame_format not in RGB_FRAME_FORMATS + tuple(YUV_SHIFTS) + tuple(YUV16_FORMATS) + tuple(BAYER_FORMATS):
        # (the text up to here is as it was; a name that reads like a Bayer format gets the Bayer names appended)
        bayer = isinstance(rgb_frame_format, str) and rgb_frame_format.lower().startswith("bayer")
        raise ValueError("rgb_frame_format must be 'interleaved' or 'nv12', or 'p010' / 'p012' / 'p016', or 'yuv420' / 'yuv422' / "
                         "'yuv444', got %r (or, for uint16 planes, 'yuvXp10' / 'yuvXp12' / 'yuvXp10msb' / 'yuvXp12msb' / 'yuvXp16' with X "
                         "one of 420, 422, 444)%s" % (rgb_frame_format, " (or, for raw Bayer mosaics, 'bayer_rggb' / 'bayer_grbg' / 'bayer_gbrg' / "
                                                      "'bayer_bggr'; util.zoom.BAYER_LAYOUTS maps the GenICam names)" if bayer else ""))
    if rgb_frame_format in BAYER_FORMATS:
        name = "rgb_frame_format=%r" % (rgb_frame_format,)
        if mode != "rgb":
            raise ValueError("%s is for mode 'rgb' (a gray value from a mosaic is not provided)" % name)
        if rgb_frame_dtype != "float32":
            raise ValueError("%s does not combine with rgb_frame_dtype=%r (the mosaic is uint8, one byte per pixel; the converted "
                             "channels are float32)" % (name, rgb_frame_dtype))
        if rgb_frame_layout != "packed":
            raise ValueError("%s does not combine with rgb_frame_layout=%r (the mosaic carries its own strides)" % (name, rgb_frame_layout))
        if frame_dtype != "float32":
            raise ValueError("%s does not combine with frame_dtype=%r (frame_dtype describes the frames of mode 'gray')" % (name, frame_dtype))
        if frame_channels != 1:
            raise ValueError("%s does not combine with frame_channels=%r (frame_channels describes the frames of mode 'gray')"
                             % (name, frame_channels))
        if frame_layout != "packed":
            raise ValueError("%s does not combine with frame_layout=%r (frame_layout describes the frames of mode 'gray')" % (name, frame_layout))
        if hw is not None and min(int(hw[0]), int(hw[1])) < 2:
            raise ValueError("%s needs H and W of at least 2, got %s" % (name, tuple(int(v) for v in hw)))
        return rgb_frame_format
    if rgb_frame_format != "interleaved":
        name = "rgb_frame_format=%r" % (rgb_frame_format,)
        src, sx, sy = rgb_source(rgb_frame_format)[:3]
        wide = src.elem == 2
        if mode != "rgb":
            raise ValueError("%s is for mode 'rgb' (mode 'gray' reads the luma plane through frame_layout='strided'%s)"
                             % (name, " with frame_dtype='uint16'" if wide else ""))
        if rgb_frame_dtype != "float32":
            raise ValueError("%s does not combine with rgb_frame_dtype=%r (the planes are %s; the converted "
                             "channels are float32)" % (name, rgb_frame_dtype, src.dtype))
        if rgb_frame_layout != "packed":
            raise ValueError("%s does not combine with rgb_frame_layout=%r (the planes carry their own pitches)" % (name, rgb_frame_layout))
        if frame_dtype != "float32":
            raise ValueError("%s does not combine with frame_dtype=%r (frame_dtype describes the frames of mode 'gray')" % (name, frame_dtype))
        if frame_channels != 1:
            raise ValueError("%s does not combine with frame_channels=%r (frame_channels describes the frames of mode 'gray')"
                             % (name, frame_channels))
        if frame_layout != "packed":
            raise ValueError("%s does not combine with frame_layout=%r (frame_layout describes the frames of mode 'gray')" % (name, frame_layout))
        # (a pair is 4:2:0: sx = sy = 1, and an even extent >= 1 is >= 2)
        if hw is not None and ((sy and int(hw[0]) % 2) or (sx and int(hw[1]) % 2) or min(int(hw[0]), int(hw[1])) < 1):
            raise ValueError("%s needs even %s, got %s" % (name, "H and W (4:2:0 chroma)" if sy else "W (4:2:2 chroma)",
                                                          tuple(int(v) for v in hw)))
    return rgb_frame_format


def nv12_coefficients(nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr"):
    """(m, oy) of the NV12 entry points: m [3, 3] float32, row k = output channel k over (Y - oy, U - 128, V - 128), and oy float32.
    nv12_matrix: "bt601" / "bt709" -- built in float64 from (Kr, Kb), each coefficient rounded once to float32:
        R = ys Y' + 2 (1 - Kr) cs V',  B = ys Y' + 2 (1 - Kb) cs U',  G = ys Y' - 2 Kb (1 - Kb) / Kg cs U' - 2 Kr (1 - Kr) / Kg cs V'
    with (ys, cs, oy) = (255 / 219, 255 / 224, 16) for nv12_range="limited" and (1, 1, 0) for "full", rows in nv12_order ("bgr" /
    "rgb") -- or a 3 x 3 array-like taken as it is (rows = output channels; nv12_order is not applied), nv12_range giving oy."""
    if nv12_range not in NV12_RANGES:
        raise ValueError("nv12_range must be 'limited' or 'full', got %r" % (nv12_range,))
    if nv12_order not in NV12_ORDERS:
        raise ValueError("nv12_order must be 'bgr' or 'rgb', got %r" % (nv12_order,))
    ys, cs, oy = (255.0 / 219.0, 255.0 / 224.0, 16.0) if nv12_range == "limited" else (1.0, 1.0, 0.0)
    if isinstance(nv12_matrix, str):
        if nv12_matrix not in NV12_MATRICES:
            raise ValueError("nv12_matrix must be 'bt601', 'bt709' or a 3 x 3 array, got %r" % (nv12_matrix,))
        kr, kb = NV12_MATRICES[nv12_matrix]
        kg = 1.0 - kr - kb
        rows = {"r": (ys, 0.0, 2.0 * (1.0 - kr) * cs),
                "g": (ys, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs),
                "b": (ys, 2.0 * (1.0 - kb) * cs, 0.0)}
        m = np.array([rows[c] for c in nv12_order], np.float64)
    else:
        try:
            m = np.array(nv12_matrix, np.float64)
        except (TypeError, ValueError):
            raise ValueError("nv12_matrix must be 'bt601', 'bt709' or a 3 x 3 array, got %r" % (nv12_matrix,))
        if m.shape != (3, 3) or not np.all(np.isfinite(m)):
            raise ValueError("nv12_matrix must be 'bt601', 'bt709' or a finite 3 x 3 array, got shape %s" % (m.shape,))
    return m.astype(np.float32), np.float32(oy)


def p010_coefficients(nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr", depth=10):
    """(m, oy, oc) of the P010 entry points for code values of ``depth`` bits (10, 12, 16): m [3, 3] float32, row k = output channel k
    over (Y - oy, U - oc, V - oc), oy and oc float32.  With s = 2^(depth - 8): nv12_matrix "bt601" / "bt709" / "bt2020" -- the rows of
    nv12_coefficients built in float64 from (Kr, Kb), each coefficient rounded once to float32, with (ys, cs, oy, oc) =
    (255 / (219 s), 255 / (224 s), 16 s, 128 s) for nv12_range="limited" and (255 / (2^depth - 1), 255 / (2^depth - 1), 0, 128 s) for
    "full", rows in nv12_order -- or a 3 x 3 array-like of coefficients ON THE 8-BIT SCALE, as for NV12 (rows = output channels;
    nv12_order is not applied): it is multiplied by 2^-(depth - 8), which is exact, and nv12_range gives oy (16 s or 0)."""
    if depth not in (10, 12, 16):
        raise ValueError("depth must be 10, 12 or 16, got %r" % (depth,))
    if nv12_range not in NV12_RANGES:
        raise ValueError("nv12_range must be 'limited' or 'full', got %r" % (nv12_range,))
    if nv12_order not in NV12_ORDERS:
        raise ValueError("nv12_order must be 'bgr' or 'rgb', got %r" % (nv12_order,))
    s = float(2 ** (depth - 8))
    full = 255.0 / (2.0 ** depth - 1.0)
    ys, cs, oy = (255.0 / (219.0 * s), 255.0 / (224.0 * s), 16.0 * s) if nv12_range == "limited" else (full, full, 0.0)
    if isinstance(nv12_matrix, str):
        if nv12_matrix not in P010_MATRICES:
            raise ValueError("nv12_matrix must be 'bt601', 'bt709', 'bt2020' or a 3 x 3 array, got %r" % (nv12_matrix,))
        kr, kb = P010_MATRICES[nv12_matrix]
        kg = 1.0 - kr - kb
        rows = {"r": (ys, 0.0, 2.0 * (1.0 - kr) * cs),
                "g": (ys, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs),
                "b": (ys, 2.0 * (1.0 - kb) * cs, 0.0)}
        m = np.array([rows[c] for c in nv12_order], np.float64).astype(np.float32)
    else:
        try:
            m = np.array(nv12_matrix, np.float64)
        except (TypeError, ValueError):
            raise ValueError("nv12_matrix must be 'bt601', 'bt709', 'bt2020' or a 3 x 3 array, got %r" % (nv12_matrix,))
        if m.shape != (3, 3) or not np.all(np.isfinite(m)):
            raise ValueError("nv12_matrix must be 'bt601', 'bt709', 'bt2020' or a finite 3 x 3 array, got shape %s" % (m.shape,))
        m = m.astype(np.float32) * np.float32(1.0 / s)          # (a power of two: exact)
    return m, np.float32(oy), np.float32(128.0 * s)


# The YUV-family colour sources, ONE description each: kind (the stem of its entry points, silent_pyramid_<kind> / silent_<kind>_to_rgb,
# and of _lib.<kind>_ptr), the name its messages use, planes (2: a pair (y, uv); 3: a triple (y, u, v)), the bytes and dtype of an
# element, its coefficient function, and whether torch CPU tensors pass as host planes (16-bit YUV alone accepts them).  A fifth format
# adds a row here and its names to rgb_source.
RgbSource = collections.namedtuple("RgbSource", "kind name planes elem dtype coefficients cpu_tensors")
RGB_SOURCES = dict((s.kind, s) for s in (RgbSource("nv12", "NV12", 2, 1, "uint8", nv12_coefficients, False),
                                         RgbSource("p010", "P010", 2, 2, "uint16", p010_coefficients, False),
                                         RgbSource("yuv", "YUV", 3, 1, "uint8", nv12_coefficients, False),
                                         RgbSource("yuv16", "16-bit YUV", 3, 2, "uint16", p010_coefficients, True)))


def rgb_source(rgb_frame_format):
    """(source, sx, sy, depth, shift) of a valid rgb_frame_format -- the format's description and parameters: chroma shifts, bits of a
    code value, bits below it -- or None for "interleaved"."""
    if rgb_frame_format == "nv12":
        return RGB_SOURCES["nv12"], 1, 1, 8, 0
    if rgb_frame_format in P010_DEPTHS:
        return RGB_SOURCES["p010"], 1, 1, P010_DEPTHS[rgb_frame_format], 16 - P010_DEPTHS[rgb_frame_format]
    if rgb_frame_format in YUV_SHIFTS:
        return (RGB_SOURCES["yuv"],) + YUV_SHIFTS[rgb_frame_format] + (8, 0)
    if rgb_frame_format in YUV16_FORMATS:
        return (RGB_SOURCES["yuv16"],) + YUV16_FORMATS[rgb_frame_format]
    return None


def _plane_geometry(src, p):
    """(shape, BYTE strides, address) of one plane of a source; its dtype must be the source's (nothing is converted)."""
    text = "%s planes must be %s GPU tensors or %s ndarrays (nothing is converted), got %s" % (src.name, src.dtype, src.dtype, p.dtype)
    if is_torch_tensor(p):
        import torch
        if p.dtype != getattr(torch, src.dtype) or not (p.is_cuda or src.cpu_tensors):
            raise ValueError(text)
        return tuple(int(s) for s in p.shape), tuple(src.elem * int(s) for s in p.stride()), int(p.data_ptr())
    if p.dtype != np.dtype(src.dtype):
        raise ValueError(text)
    return tuple(int(s) for s in p.shape), tuple(int(s) for s in p.strides), int(p.ctypes.data)


def _pair_fields(src, geo, h, w):
    """(y address, uv address, y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride) and n of a pair (y, uv): y [n, H, W] with
    adjacent elements, uv [n, H / 2, W / 2, 2] with the two elements of a pair and the pairs of a row adjacent, positive
    non-overlapping row / frame strides (BYTES; e: the bytes of an element)."""
    (ys, yst, ya), (cs, cst, ca) = geo
    e, strides = src.elem, "strides" if src.elem == 1 else "byte strides"
    if len(ys) != 3 or ys[1:] != (h, w) or ys[0] < 1:
        raise ValueError("the %s luma plane must be [n, %d, %d], got %s" % (src.name, h, w, ys))
    n = ys[0]
    if cs != (n, h // 2, w // 2, 2):
        raise ValueError("the %s chroma plane must be [%d, %d, %d, 2], got %s" % (src.name, n, h // 2, w // 2, cs))
    if (w > 1 and yst[2] != e) or cst[3] != e or (w > 2 and cst[2] != 2 * e):
        raise ValueError("%s planes: luma %s of a row and the (U, V) pairs of a chroma row must be adjacent (%s %s, %s)"
                         % (src.name, "bytes" if e == 1 else "elements", strides, yst, cst))
    yr, cr = (yst[1] if h > 1 else e * w), (cst[1] if h > 2 else e * w)
    yf, cf = (yst[0] if n > 1 else (h - 1) * yr + e * w), (cst[0] if n > 1 else (h // 2 - 1) * cr + e * w)
    if yr < e * w or cr < e * w or yf < (h - 1) * yr + e * w or cf < (h // 2 - 1) * cr + e * w:
        raise ValueError("%s planes: rows or frames overlap, or a stride is not positive (%s %s, %s)" % (src.name, strides, yst, cst))
    return (ya, ca, yr, yf, cr, cf), n


def _triple_fields(src, geo, h, w, sx, sy, fmt):
    """(y, u, v addresses, y_pixel_stride, y_row_stride, y_frame_stride, c_pixel_stride, c_row_stride, c_frame_stride) and n of a triple
    (y, u, v): y [n, H, W], u and v [n, H >> sy, W >> sx]; each ANY view with positive strides, u and v with EQUAL strides (BYTES; e:
    the bytes of an element, uint16 elements at even addresses and strides)."""
    (ys, yst, ya), (us, ust, ua), (vs, vst, va) = geo
    e, strides = src.elem, "strides" if src.elem == 1 else "byte strides"
    if len(ys) != 3 or ys[1:] != (h, w) or ys[0] < 1:
        raise ValueError("the %s luma plane must be [n, %d, %d], got %s" % (src.name, h, w, ys))
    n = ys[0]
    ch, cw = h >> sy, w >> sx
    if us != (n, ch, cw) or vs != (n, ch, cw):
        raise ValueError("the %s chroma planes must be [%d, %d, %d], got %s and %s" % (fmt, n, ch, cw, us, vs))

    def fields(st, rows, cols):
        # (a stride of an axis of extent 1 is never used: the smallest legal value stands in for it)
        px = st[2] if cols > 1 else e
        row = st[1] if rows > 1 else (cols - 1) * px + e
        frame = st[0] if n > 1 else (rows - 1) * row + (cols - 1) * px + e
        return px, row, frame

    yp, yr, yf = fields(yst, h, w)
    cp, cr, cf = fields(ust, ch, cw)
    if fields(vst, ch, cw) != (cp, cr, cf):
        raise ValueError("%s planes: u and v must have equal strides, got %s and %s" % (src.name, ust, vst))
    if min(yp, cp) < e or yr < (w - 1) * yp + e or cr < (cw - 1) * cp + e or yf < (h - 1) * yr + (w - 1) * yp + e \
            or cf < (ch - 1) * cr + (cw - 1) * cp + e:
        raise ValueError("%s planes: rows or frames overlap, or a stride is not positive (%s %s, %s)" % (src.name, strides, yst, ust))
    if e == 2 and (yp | yr | yf | cp | cr | cf | ya | ua | va) & 1:
        raise ValueError("%s planes: an address or a byte stride is odd (uint16 elements; byte strides %s, %s)" % (src.name, yst, ust))
    return (ya, ua, va, yp, yr, yf, cp, cr, cf), n


def rgb_source_frames_of(src, planes, hw, coeffs, sx=1, sy=1, depth=8, shift=0, fmt=None):
    """The planes of a source -- all GPU tensors, or all ndarrays (torch CPU tensors too where the source takes them) -- as what
    _lib.<kind>_ptr takes: the fields of the struct in their order, coeffs = (m, oy[, oc]).  Returns (that tuple, n, on_device).
    Nothing is converted or copied."""
    if not isinstance(planes, (tuple, list)) or len(planes) != src.planes:
        raise ValueError("%s frames are a %s of %s planes" % (src.name, "pair (y, uv)" if src.planes == 2 else "triple (y, u, v)", src.dtype))
    # (GPU tensors: read in place on the device; ndarrays -- and torch CPU tensors, 16-bit YUV -- host memory, staged by the host forms)
    dev = all(is_torch_tensor(p) and (p.is_cuda or not src.cpu_tensors) for p in planes)
    if not dev and not all(isinstance(p, np.ndarray) or (src.cpu_tensors and is_torch_tensor(p) and not p.is_cuda) for p in planes):
        raise TypeError(TYPE_ERROR_MESSAGE)
    h, w = int(hw[0]), int(hw[1])
    geo = [_plane_geometry(src, p) for p in planes]
    tail = ([float(c) for c in np.asarray(coeffs[0], np.float32).reshape(9)],) + tuple(float(c) for c in coeffs[1:])
    if src.planes == 2:
        fields, n = _pair_fields(src, geo, h, w)
        return fields + tail + ((shift,) if src.elem == 2 else ()), n, dev
    fields, n = _triple_fields(src, geo, h, w, sx, sy, fmt)
    return fields + (sx, sy) + tail + ((shift, depth) if src.elem == 2 else ()), n, dev


def nv12_frames_of(planes, hw, m, oy):
    """A pair (y, uv) of uint8 planes -- both ndarrays or both GPU tensors; y [n, H, W] with element stride 1, uv [n, H / 2, W / 2, 2]
    with strides (.., .., 2, 1), positive row / frame strides -- as what _lib.nv12_ptr takes: (y address, uv address, y_row_stride,
    y_frame_stride, uv_row_stride, uv_frame_stride, m, oy).  Returns (that tuple, n, on_device).  Nothing is converted or copied."""
    return rgb_source_frames_of(RGB_SOURCES["nv12"], planes, hw, (m, oy))


def p010_frames_of(planes, hw, m, oy, oc, depth):
    """The same pair as uint16 planes -- both ndarrays or both torch.uint16 GPU tensors -- as what _lib.p010_ptr takes: (y address, uv
    address, y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride (BYTES), m, oy, oc, shift = 16 - depth).  Returns (that tuple,
    n, on_device)."""
    if depth not in (10, 12, 16):
        raise ValueError("depth must be 10, 12 or 16, got %r" % (depth,))
    return rgb_source_frames_of(RGB_SOURCES["p010"], planes, hw, (m, oy, oc), depth=depth, shift=16 - depth)


def yuv_frames_of(planes, hw, fmt, m, oy):
    """A triple (y, u, v) of uint8 planes -- all ndarrays or all GPU tensors; y [n, H, W], u and v [n, H >> sy, W >> sx] with (sx, sy)
    = YUV_SHIFTS[fmt]; each ANY view with positive strides (the layout lives in the strides: yuyv[:, :, 0::2], yuyv[:, :, 1::4],
    yuyv[:, :, 3::4] is a valid triple), u and v with EQUAL strides -- as what _lib.yuv_ptr takes: (y, u, v addresses, y_pixel_stride,
    y_row_stride, y_frame_stride, c_pixel_stride, c_row_stride, c_frame_stride (BYTES), sx, sy, m, oy).  Returns (that tuple, n,
    on_device)."""
    if fmt not in YUV_SHIFTS:
        raise ValueError("fmt must be 'yuv420', 'yuv422' or 'yuv444', got %r" % (fmt,))
    return rgb_source_frames_of(RGB_SOURCES["yuv"], planes, hw, (m, oy), *YUV_SHIFTS[fmt], fmt=fmt)


def yuv16_frames_of(planes, hw, fmt, m, oy, oc):
    """The same triple as uint16 planes -- all torch.uint16 GPU tensors, or all host arrays (ndarrays or torch CPU tensors) -- with
    (sx, sy, depth, shift) = YUV16_FORMATS[fmt] (y210[:, :, 0::2], y210[:, :, 1::4], y210[:, :, 3::4] is a valid triple), as what
    _lib.yuv16_ptr takes: (y, u, v addresses, y_pixel_stride, y_row_stride, y_frame_stride, c_pixel_stride, c_row_stride, c_frame_stride
    (BYTES, even), sx, sy, m, oy, oc, shift, depth).  Returns (that tuple, n, on_device)."""
    if fmt not in YUV16_FORMATS:
        raise ValueError("fmt must be one of %s, got %r" % (", ".join(sorted(YUV16_FORMATS)), fmt))
    return rgb_source_frames_of(RGB_SOURCES["yuv16"], planes, hw, (m, oy, oc), *YUV16_FORMATS[fmt], fmt=fmt)


def source_frames_of(fmt, planes, hw, nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr"):
    """(source, frames_of result) of a batch of a valid rgb_frame_format other than "interleaved": the coefficients of the format
    (nv12_coefficients; p010_coefficients at the format's depth for uint16 planes), then its *_frames_of."""
    src, sx, sy, depth, shift = rgb_source(fmt)
    coeffs = src.coefficients(nv12_matrix, nv12_range, nv12_order, *((depth,) if src.elem == 2 else ()))
    return src, rgb_source_frames_of(src, planes, hw, coeffs, sx, sy, depth, shift, fmt)


class _SourceOperand(_Operand):
    """A batch of a YUV-family source (the result of its *_frames_of) as an operand: results are allocated like the planes (empty) and
    the entry point is called in its _dev form on torch's current stream for GPU planes, in its host form otherwise (call)."""

    def __init__(self, src, planes, hw, frames, ctx=None):
        args, self.n_frames, self.dev = frames
        self.kind = src.kind
        self.packed, self.c, self.extents = False, 3, [(int(hw[0]), int(hw[1]))]
        self.device = self.stream = None
        if self.dev:
            import torch
            self._torch_device = planes[0].device
            self.device = self._torch_device.index or 0
            self.stream = C.c_void_p(torch.cuda.current_stream(self._torch_device).cuda_stream)
        self.ptr = getattr(_lib, src.kind + "_ptr")(args)
        self.buf = tuple(planes)                        # keep alive
        self.ctx = ctx or get_context(self.device)


def _to_rgb(kind, fmt, planes, hw, frames_of, device):
    """The float32 frames [n, H, W, 3] the pyramid kernels see for a batch of format ``fmt`` (silent_<kind>_to_rgb[_dev]: the loaders'
    own device functions, one thread per pixel), on the 0 .. 255 scale and not rounded."""
    check_rgb_frame_format(fmt, hw=hw)
    op = _SourceOperand(RGB_SOURCES[kind], planes, hw, frames_of(), None if device is None else get_context(device))
    h, w = int(hw[0]), int(hw[1])
    out, optr = op.empty((op.n_frames, h, w, 3))
    op.call(kind + "_to_rgb", op.ptr, op.n_frames, h, w, optr)
    return out


def nv12_to_rgb(planes, hw, nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr", device=None):
    """_to_rgb for an NV12 batch -- for display, and as the reference of the bit-identity contract.  planes: nv12_frames_of."""
    m, oy = nv12_coefficients(nv12_matrix, nv12_range, nv12_order)
    return _to_rgb("nv12", "nv12", planes, hw, lambda: nv12_frames_of(planes, hw, m, oy), device)


def p010_to_rgb(planes, hw, depth=10, nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr", device=None):
    """_to_rgb for a P010 (depth=10) / P012 (12) / P016 (16) batch.  planes: p010_frames_of."""
    m, oy, oc = p010_coefficients(nv12_matrix, nv12_range, nv12_order, depth)
    return _to_rgb("p010", {10: "p010", 12: "p012", 16: "p016"}[depth], planes, hw, lambda: p010_frames_of(planes, hw, m, oy, oc, depth), device)


def yuv_to_rgb(planes, hw, fmt="yuv420", nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr", device=None):
    """_to_rgb for a (y, u, v) triple of format ``fmt`` ("yuv420" / "yuv422" / "yuv444").  planes: yuv_frames_of; the conversion:
    nv12_coefficients."""
    m, oy = nv12_coefficients(nv12_matrix, nv12_range, nv12_order)
    return _to_rgb("yuv", fmt, planes, hw, lambda: yuv_frames_of(planes, hw, fmt, m, oy), device)


def yuv16_to_rgb(planes, hw, fmt="yuv420p10", nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr", device=None):
    """_to_rgb for a (y, u, v) triple of uint16 views of format ``fmt`` (one of YUV16_FORMATS).  planes: yuv16_frames_of; the
    conversion: p010_coefficients at the format's depth."""
    if fmt not in YUV16_FORMATS:
        raise ValueError("fmt must be one of %s, got %r" % (", ".join(sorted(YUV16_FORMATS)), fmt))
    m, oy, oc = p010_coefficients(nv12_matrix, nv12_range, nv12_order, YUV16_FORMATS[fmt][2])
    return _to_rgb("yuv16", fmt, planes, hw, lambda: yuv16_frames_of(planes, hw, fmt, m, oy, oc), device)


# Raw Bayer mosaics: neither a pair nor a triple -- ONE uint8 view -- so a description outside RGB_SOURCES (kind: the stem of
# silent_pyramid_bayer / silent_bayer_to_rgb and of _lib.bayer_ptr) and functions of its own.
BAYER_SOURCE = RgbSource("bayer", "Bayer", 1, 1, "uint8", None, False)


def check_bayer_conversion(rgb_frame_format, nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr"):
    """The nv12_* keywords beside a Bayer rgb_frame_format: nv12_order selects the channel order as for every other source ("bgr" ->
    0, "rgb" -> 1: returned); a non-default nv12_matrix or nv12_range is refused -- a mosaic has no YUV matrix and no range, the
    keyword would silently mean nothing."""
    name = "rgb_frame_format=%r" % (rgb_frame_format,)
    if not (isinstance(nv12_matrix, str) and nv12_matrix == "bt709"):
        raise ValueError("%s does not combine with nv12_matrix (a Bayer mosaic is demosaiced, no YUV matrix is applied)" % name)
    if not (isinstance(nv12_range, str) and nv12_range == "limited"):
        raise ValueError("%s does not combine with nv12_range=%r (a Bayer mosaic has no YUV range)" % (name, nv12_range))
    if nv12_order not in NV12_ORDERS:
        raise ValueError("nv12_order must be 'bgr' or 'rgb', got %r" % (nv12_order,))
    return NV12_ORDERS.index(nv12_order)


def bayer_frames_of(frames, hw, fmt, nv12_order="bgr"):
    """A batch of raw 8-bit Bayer mosaics -- a uint8 ndarray or a uint8 GPU tensor [n, H, W] or [n, H, W, 1], ANY view with positive
    strides (a pitched buffer, a window of a larger sensor image, every second byte); ``fmt`` (one of BAYER_FORMATS) names the top-left
    2 x 2 cell of THIS view -- as what _lib.bayer_ptr takes: (address, pixel_stride, row_stride, frame_stride (BYTES), pattern, order).
    Returns (that tuple, n, on_device).  Nothing is converted or copied."""
    if fmt not in BAYER_FORMATS:
        raise ValueError("fmt must be one of %s, got %r" % (", ".join(BAYER_FORMATS), fmt))
    order = check_bayer_conversion(fmt, nv12_order=nv12_order)
    dev = is_torch_tensor(frames)
    if not dev and not isinstance(frames, np.ndarray):
        raise TypeError(TYPE_ERROR_MESSAGE)
    h, w = int(hw[0]), int(hw[1])
    if min(h, w) < 2:
        raise ValueError("rgb_frame_format=%r needs H and W of at least 2, got %s" % (fmt, (h, w)))
    shape, st, address = _plane_geometry(BAYER_SOURCE, frames)
    if len(shape) == 4 and shape[3] == 1:
        shape, st = shape[:3], st[:3]
    if len(shape) != 3 or shape[1:] != (h, w) or shape[0] < 1:
        raise ValueError("a Bayer mosaic batch must be [n, %d, %d] or [n, %d, %d, 1], got %s" % (h, w, h, w, tuple(int(s) for s in frames.shape)))
    n = shape[0]
    # (a stride of an axis of extent 1 is never used: the smallest legal value stands in for it)
    ps, rs = st[2], st[1]
    fs = st[0] if n > 1 else (h - 1) * rs + (w - 1) * ps + 1
    if ps < 1 or rs < (w - 1) * ps + 1 or fs < (h - 1) * rs + (w - 1) * ps + 1:
        raise ValueError("Bayer mosaics: rows or frames overlap, or a stride is not positive (strides %s)" % (st,))
    return (address, ps, rs, fs, BAYER_FORMATS[fmt], order), n, dev


def bayer_to_rgb(frames, hw, fmt, nv12_order="bgr", device=None):
    """The float32 frames [n, H, W, 3] the pyramid kernels see for a batch of Bayer mosaics of format ``fmt`` (silent_bayer_to_rgb[_dev]:
    the loaders' own device function, one thread per pixel): bilinear demosaicing on the 0 .. 255 scale, multiples of 1/4, not rounded
    -- for display, and as the reference of the bit-identity contract.  frames: bayer_frames_of.  This is not OpenCV's
    COLOR_Bayer*2BGR (which rounds to uint8 and treats borders differently), and OpenCV's pattern names are shifted against the
    sensor's."""
    args = bayer_frames_of(frames, hw, fmt, nv12_order)
    op = _SourceOperand(BAYER_SOURCE, (frames,), hw, args, None if device is None else get_context(device))
    h, w = int(hw[0]), int(hw[1])
    out, optr = op.empty((op.n_frames, h, w, 3))
    op.call("bayer_to_rgb", op.ptr, op.n_frames, h, w, optr)
    return out


class PyramidPlan(object):
    """Tap tables of one (frame size, level geometry) on the device.  ``levels`` is a list of dicts / tuples
    (src_y0, src_x0, src_h, src_w, zoom_h, zoom_w, out_h, out_w).  accumulation="float64" (single-channel plans): every op of
    run / gray_pass / gray_keypoints sums its taps in float64 and rounds once, like the CPU oracle (SILENT_PLAN_ACCUM_F64)."""

    def __init__(self, frame_h, frame_w, channels, levels, device=None, accumulation="float32"):
        self.accumulation = check_accumulation(accumulation)
        self.ctx = get_context(device)
        self.frame_shape = (int(frame_h), int(frame_w), int(channels))
        self.levels = [tuple(int(v) for v in l) for l in levels]
        self.extents = [(l[6], l[7]) for l in self.levels]
        arr = (_lib.PyrLevel * len(self.levels))(*[_lib.PyrLevel(*l) for l in self.levels])
        self.handle = C.c_void_p()
        flags = _lib.PLAN_ACCUM_F64 if accumulation == "float64" else 0
        self.ctx.check(_lib.load().silent_pyramid_plan_create_ex(self.ctx.handle, self.frame_shape[0], self.frame_shape[1],
                                                                 self.frame_shape[2], arr, len(self.levels), flags,
                                                                 C.byref(self.handle)))
        self.frame_px = sum(h * w for h, w in self.extents)

    def _frames(self, frames, frame_dtype="float32", frame_channels=1, frame_layout="packed"):
        """[n, H, W, C] frames of this plan (ndarray, or torch GPU tensor) as an operand on the plan's context.  frame_dtype="uint8":
        a uint8 ndarray or contiguous uint8 GPU tensor, passed as it is (anything else is a ValueError); "float32": widened.
        frame_channels=3 (single-channel plans, uint8): the frames are [n, H, W, 3] interleaved colour.  frame_layout="strided"
        (uint8 / uint16): any view with positive strides (frame_view_of), passed as it is; [n, H, W] does for one channel.
        frame_dtype="uint16": as "uint8" with unsigned 16-bit elements, one channel."""
        mode = "gray" if self.frame_shape[2] == 1 else "rgb"
        check_frame_channels(frame_channels, mode, frame_dtype, self.accumulation)      # (first: a refused 3 is reported as such)
        check_frame_dtype(frame_dtype, mode, self.accumulation)
        check_frame_layout(frame_layout, mode, frame_dtype, self.accumulation)
        if not (isinstance(frames, np.ndarray) or is_torch_tensor(frames)):
            raise TypeError(TYPE_ERROR_MESSAGE)
        if frame_layout == "strided" and frame_channels == 1 and frames.ndim == 3:
            frames = frames[..., None]
        shape = self.frame_shape[:2] + (3,) if frame_channels == 3 else self.frame_shape
        if tuple(frames.shape[1:]) != shape:
            raise ValueError("frames must be [n, %d, %d, %d], got %s" % (shape + (tuple(frames.shape),)))
        return _Operand(frames, ctx=self.ctx, frame_dtype=frame_dtype, frame_layout=frame_layout)

    @staticmethod
    def _entry(name, frame_dtype, frame_channels, frame_layout="packed"):
        """The entry point family of a frame layout: silent_<name>, silent_<name>_u8, silent_<name>_u8x3, silent_<name>_view,
        silent_<name>_u16 or silent_<name>_view16."""
        return _lib.gray_entry(name, frame_dtype, frame_channels, frame_layout=frame_layout)[0]

    def _frames_rgb8(self, frames):
        """[n, H, W, 3] packed uint8 colour frames of this 3-channel plan (uint8 ndarray, or contiguous uint8 GPU tensor) as an
        operand on the plan's context: passed as they are, anything else is refused, never converted."""
        _require_narrow(frames, "uint8")
        if frames.ndim != 4 or tuple(frames.shape[1:]) != self.frame_shape:
            raise ValueError("frames must be [n, %d, %d, %d], got %s" % (self.frame_shape + (tuple(frames.shape),)))
        return _Operand(frames, ctx=self.ctx, frame_dtype="uint8")

    def _frames_rgb8_view(self, frames):
        """[n, H, W, 3] uint8 colour frames of this 3-channel plan as ANY view with positive strides and channel stride 1 (uint8
        ndarray or uint8 GPU tensor; frame_view_of), passed as it is: a ValueError for another dtype, shape or channel stride and for
        flipped, broadcast or overlapping views; nothing is converted or copied."""
        if not (isinstance(frames, np.ndarray) or is_torch_tensor(frames)):
            raise TypeError(TYPE_ERROR_MESSAGE)
        if frames.ndim != 4 or tuple(frames.shape[1:]) != self.frame_shape:
            raise ValueError("frames must be [n, %d, %d, %d], got %s" % (self.frame_shape + (tuple(frames.shape),)))
        return _Operand(frames, ctx=self.ctx, frame_dtype="uint8", frame_layout="strided")

    def run(self, frames, frame_dtype="float32", frame_channels=1, frame_layout="packed", rgb_frame_dtype="float32",
            rgb_frame_layout="packed", rgb_frame_format="interleaved", nv12_matrix="bt709", nv12_range="limited", nv12_order="bgr"):
        """frames: [n, H, W, C] ndarray (host) or torch GPU tensor.  Returns a PackedPyramid.  frame_dtype="uint8" (single-channel
        plans): uint8 frames read as they are (silent_pyramid_u8), the same pyramid bit for bit.  frame_channels=3 (with "uint8"):
        [n, H, W, 3] interleaved colour frames (silent_pyramid_u8x3), the pyramid of the frame of values (b0 + b1 + b2) * f32(1/3).
        frame_layout="strided" (with "uint8"): any uint8 view with positive strides, read in place (silent_pyramid_view).
        frame_dtype="uint16": unsigned 16-bit frames read as they are (silent_pyramid_u16; strided: silent_pyramid_view16), the pyramid of
        frames.astype(float32) bit for bit.
        rgb_frame_dtype="uint8" (3-channel plans): packed uint8 colour frames [n, H, W, 3] read as they are (silent_pyramid_rgb8),
        the 3-channel pyramid of frames.astype(float32) bit for bit.  rgb_frame_layout="strided" (with rgb_frame_dtype="uint8"): any
        uint8 view [n, H, W, 3] with positive strides and channel stride 1, read in place (silent_pyramid_rgb8_view), the pyramid of the
        packed uint8 call on the compacted view bit for bit.  rgb_frame_format="nv12" (3-channel plans): frames is a pair (y, uv) of
        uint8 planes (nv12_frames_of) read in place and converted in registers (silent_pyramid_nv12; nv12_coefficients), the pyramid
        of the float32 call on nv12_to_rgb(frames) bit for bit.  rgb_frame_format="yuv420" / "yuv422" / "yuv444": frames is a triple
        (y, u, v) of uint8 views of any positive strides (yuv_frames_of; silent_pyramid_yuv), the pyramid of the float32 call on
        yuv_to_rgb(frames, hw, fmt) bit for bit.  rgb_frame_format one of YUV16_FORMATS ("yuv420p10" ...): the same triple as uint16
        views (yuv16_frames_of; silent_pyramid_yuv16; p010_coefficients at the format's depth), the pyramid of the float32 call on
        yuv16_to_rgb(frames, hw, fmt) bit for bit."""
        mode = "gray" if self.frame_shape[2] == 1 else "rgb"
        fmt = check_rgb_frame_format(rgb_frame_format, mode, rgb_frame_dtype, rgb_frame_layout, frame_dtype, frame_channels, frame_layout,
                                     self.frame_shape[:2])
        if fmt in BAYER_FORMATS:
            # a raw Bayer mosaic: ONE uint8 view [n, H, W] read in place and demosaiced in registers (silent_pyramid_bayer), the pyramid
            # of the float32 call on bayer_to_rgb(frames, hw, fmt) bit for bit.  nv12_order: the channel order; a matrix or a range
            # beside a mosaic is refused
            check_bayer_conversion(fmt, nv12_matrix, nv12_range, nv12_order)
            op = _SourceOperand(BAYER_SOURCE, (frames,), self.frame_shape[:2], bayer_frames_of(frames, self.frame_shape[:2], fmt, nv12_order), self.ctx)
            out, optr = op.empty(op.n_frames * self.frame_px * 3)
            op.call("pyramid_bayer", self.handle, op.ptr, op.n_frames, optr)
            return PackedPyramid(out, self.extents, 3, op.n_frames)
        if fmt != "interleaved":
            # a YUV-family source (rgb_source): the planes read in place (silent_pyramid_<kind>; the format's coefficients --
            # p010_coefficients also knows "bt2020"), the pyramid of the float32 call on <kind>_to_rgb(frames) bit for bit
            src, args = source_frames_of(fmt, frames, self.frame_shape[:2], nv12_matrix, nv12_range, nv12_order)
            op = _SourceOperand(src, frames, self.frame_shape[:2], args, self.ctx)
            out, optr = op.empty(op.n_frames * self.frame_px * 3)
            op.call("pyramid_" + src.kind, self.handle, op.ptr, op.n_frames, optr)
            return PackedPyramid(out, self.extents, 3, op.n_frames)
        check_rgb_frame_dtype(rgb_frame_dtype, mode, frame_dtype, frame_channels, frame_layout)
        strided = check_rgb_frame_layout(rgb_frame_layout, mode, rgb_frame_dtype, frame_dtype, frame_channels, frame_layout) == "strided"
        if rgb_frame_dtype == "uint8":
            op = self._frames_rgb8_view(frames) if strided else self._frames_rgb8(frames)
            out, optr = op.empty(op.n_frames * self.frame_px * 3)
            op.call("pyramid_rgb8_view" if strided else "pyramid_rgb8", self.handle, op.ptr, op.n_frames, optr)
            return PackedPyramid(out, self.extents, 3, op.n_frames)
        op, c = self._frames(frames, frame_dtype, frame_channels, frame_layout), self.frame_shape[2]
        out, optr = op.empty(op.n_frames * self.frame_px * c)
        op.call(self._entry("pyramid", frame_dtype, frame_channels, frame_layout), self.handle, op.ptr, op.n_frames, optr)
        return PackedPyramid(out, self.extents, c, op.n_frames)

    @property
    def flags(self):
        """The plan's SILENT_PLAN_* flags as the library reports them."""
        f = C.c_uint(0)
        self.ctx.check(_lib.load().silent_pyramid_plan_flags(self.handle, C.byref(f)))
        return int(f.value)

    @property
    def streamable(self):
        """True when silent_gray_pass takes the single-read stream kernel for this plan."""
        return bool(_lib.load().silent_pyramid_plan_is_streamable(self.handle))

    @property
    def walk_plans(self):
        """(number of walk plans, pixels per consumer wave) of a 3-channel plan; (0, 0): unit + region kernels."""
        px = C.c_int(0)
        n = _lib.load().silent_pyramid_plan_walk_plans(self.handle, C.byref(px))
        return int(n), int(px.value)

    def gray_pass(self, frames, cs_kernel, end_bank, clip_hi=255.0, storage="float32", frame_dtype="float32", frame_channels=1,
                  frame_layout="packed"):
        """Whole grayscale hot path (silent_gray_pass): frames [n,H,W,1] -> (pyramid, cs, end) PackedPyramids.
        Same results as run() + gray_line_end(), one pass less over level 0.  storage="float16" (silent_gray_pass_h): cs and end
        are float16 maps -- each element the float32 result rounded to nearest even -- and the pyramid stays float32.
        frame_dtype="uint8" (silent_gray_pass_u8): uint8 frames read as they are; the same maps bit for bit, either storage.
        frame_channels=3 (with "uint8"; silent_gray_pass_u8x3): frames [n,H,W,3] interleaved colour, each pixel entering as
        (b0 + b1 + b2) * float32(1/3) -- the maps of the float32 call on that frame of values, bit for bit.
        frame_layout="strided" (with "uint8"; silent_gray_pass_view): any uint8 view with positive strides, read in place.
        frame_dtype="uint16" (silent_gray_pass_u16; strided: silent_gray_pass_view16): unsigned 16-bit frames read as they are, the maps of
        frames.astype(float32) bit for bit.  storage="float16" keeps its rule -- the float32 result rounded to nearest even, overflow
        to +-inf: with full-range 16-bit data and clip_hi above 65504 a stored element can be +inf, as in the float32-frame call."""
        check_storage(storage, "gray" if self.frame_shape[2] == 1 else "rgb", self.accumulation)
        check_frame_channels(frame_channels, "gray" if self.frame_shape[2] == 1 else "rgb", frame_dtype, self.accumulation)
        check_frame_dtype(frame_dtype, "gray" if self.frame_shape[2] == 1 else "rgb", self.accumulation)
        check_frame_layout(frame_layout, "gray" if self.frame_shape[2] == 1 else "rgb", frame_dtype, self.accumulation)
        if self.frame_shape[2] != 1:
            raise ValueError("gray_pass needs a single-channel plan")
        cs = _kernel_arg(cs_kernel, 1)
        eb = _kernel_arg(end_bank, 1)
        if cs.shape != (3, 3, 1, 1) or eb.shape[:3] != (3, 3, 1):
            raise ValueError("gray_pass needs a [3,3,1,1] CS kernel and a [3,3,1,K] end bank")
        K = eb.shape[3]
        op = self._frames(frames, frame_dtype, frame_channels, frame_layout)
        n = op.n_frames
        name, _, map_ptr, tail = _lib.gray_entry("gray_pass", frame_dtype, frame_channels, storage, op.dev, frame_layout=frame_layout)
        dt = np.float16 if storage == "float16" else np.float32
        pyr, pp = op.empty(n * self.frame_px)
        (cso, cp), (endo, ep) = [op.empty(n * self.frame_px * ch, dt) for ch in (1, K)]
        op.call(name, self.handle, op.ptr, n, C.c_void_p(cs.ctypes.data), C.c_void_p(eb.ctypes.data), K, float(clip_hi), pp,
                map_ptr(cp.value), map_ptr(ep.value), *tail)
        P = PackedPyramid
        return P(pyr, self.extents, 1, n), P(cso, self.extents, 1, n, dtype=dt), P(endo, self.extents, K, n, dtype=dt)

    def gray_keypoints(self, frames, cs_kernel, end_bank, clip_hi=255.0, pad=2, selection=True, top_percent=0.1, regions=None,
                       cap_per_frame=None, frame_dtype="float32", frame_channels=1, frame_layout="packed"):
        """silent_gray_keypoints (host form): gray_pass + pad_inwards -> value -> [top_value_points -> NMS -> value ->]
        max_value_indices_region on the K-channel end map.  Returns (pyramid, cs, end, idx [n, cap, 4], counts [n]).
        regions: one (rH, rW) per level (default: half the level), the strides of TF1's max_pool(k = the whole level, SAME) whose
        window maxima a keypoint must reach; more than 4 windows per axis on any level runs the general path, without the sparse tail.
        frame_dtype="uint8" (silent_gray_keypoints_u8): uint8 frames read as they are, the same results.  frame_channels=3 (with
        "uint8"; silent_gray_keypoints_u8x3): [n,H,W,3] interleaved colour frames, the results of the frame of values.
        frame_layout="strided" (with "uint8"; silent_gray_keypoints_view): any uint8 view with positive strides, read in place.
        frame_dtype="uint16" (silent_gray_keypoints_u16; strided: silent_gray_keypoints_view16): unsigned 16-bit frames, the same results."""
        check_frame_channels(frame_channels, "gray" if self.frame_shape[2] == 1 else "rgb", frame_dtype, self.accumulation)
        check_frame_dtype(frame_dtype, "gray" if self.frame_shape[2] == 1 else "rgb", self.accumulation)
        check_frame_layout(frame_layout, "gray" if self.frame_shape[2] == 1 else "rgb", frame_dtype, self.accumulation)
        if self.frame_shape[2] != 1:
            raise ValueError("gray_keypoints needs a single-channel plan")
        cs = _kernel_arg(cs_kernel, 1)
        eb = _kernel_arg(end_bank, 1)
        if cs.shape != (3, 3, 1, 1) or eb.shape[:3] != (3, 3, 1):
            raise ValueError("gray_keypoints needs a [3,3,1,1] CS kernel and a [3,3,1,K] end bank")
        if regions is None:
            regions = [(max(h // 2, 1), max(w // 2, 1)) for h, w in self.extents]
        if len(regions) != len(self.extents):
            raise ValueError("need one (rH, rW) region per level")
        reg = (_lib.Extent * len(regions))(*[_lib.Extent(int(rh), int(rw)) for rh, rw in regions])
        K = eb.shape[3]
        op = self._frames(frames, frame_dtype, frame_channels, frame_layout)
        n = op.n_frames
        cap = self.frame_px if cap_per_frame is None else int(cap_per_frame)
        (pyr, pp), (cso, cp), (endo, ep) = [op.empty(n * self.frame_px * ch) for ch in (1, 1, K)]
        idx, iptr = op.empty((n, cap, 4), np.int64)
        counts, cptr = op.empty(n, np.int64)
        op.call(self._entry("gray_keypoints", frame_dtype, frame_channels, frame_layout), self.handle, op.ptr, n, C.c_void_p(cs.ctypes.data), C.c_void_p(eb.ctypes.data), K, float(clip_hi),
                pp, cp, ep, int(pad), int(selection), float(top_percent), reg, None, None, iptr, cap, cptr)
        P = PackedPyramid
        return P(pyr, self.extents, 1, n), P(cso, self.extents, 1, n), P(endo, self.extents, K, n), idx, counts

    def close(self):
        if self.handle:
            _lib.load().silent_pyramid_plan_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
