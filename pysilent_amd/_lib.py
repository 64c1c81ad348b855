"""ctypes binding of libsilent_hip.so (include/silent_hip.h) -- the only way the package reaches the GPU.

There is no CPU fallback anywhere in this package: if the shared library is missing, or no
gfx950 device is visible, the filters raise.  (The CPU oracle lives in ``oracle/`` and is test
infrastructure; nothing under ``pysilent_amd`` imports it.)
"""
import ctypes as C
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SILENT_LIB_PATH: load another build of the same library (kernel experiments: build.py --out ... -D..., scripts/ab_same_buffers.py)
LIB_PATH = os.environ.get("SILENT_LIB_PATH") or os.path.join(_HERE, "lib", "libsilent_hip.so")

SILENT_OK = 0
SILENT_E_INVALID = -1
SILENT_E_HIP = -2
SILENT_E_CAPACITY = -3
SILENT_E_UNSUPPORTED = -4
SILENT_E_NOMEM = -5

RELU = 1
CLIP = 2
PLAN_ACCUM_F64 = 1   # silent_pyramid_plan_create_ex flag: float64 accumulation inside each op
FLAT_IEEE = 0
FLAT_ZERO = 1
NMS_PRODUCT = 0
NMS_FIRED = 1
RECOVERY_CONSTANT = 1
RECOVERY_INPUT = 2
MAX_LEVELS = 16
TUNE_GRAY, TUNE_RGB, TUNE_PYRAMID = 0, 1, 2
GRAY_PART_PYRAMID, GRAY_PART_FILTER = 1, 2
DT_U8, DT_F32, DT_F64, DT_I32, DT_U16, DT_I16, DT_I64 = 0, 1, 2, 3, 4, 5, 6
ABI_VERSION = 5


class Extent(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32)]


class PyrLevel(C.Structure):
    _fields_ = [("src_y0", C.c_int32), ("src_x0", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32),
                ("zoom_h", C.c_int32), ("zoom_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32)]


class RgbChainParams(C.Structure):
    _fields_ = [("rgc", C.POINTER(C.c_float)), ("rgby", C.POINTER(C.c_float)), ("stripe", C.POINTER(C.c_float)),
                ("blur", C.POINTER(C.c_float)), ("end", C.POINTER(C.c_float)),
                ("regulation_value", C.c_float), ("regulation_root", C.c_float), ("flat_policy", C.c_int32),
                ("clip_hi", C.c_float), ("pad", C.c_int32)]


class BoostingParams(C.Structure):
    _fields_ = [("exhaustion_max", C.c_float), ("excitation_max", C.c_float), ("recovery_mode", C.c_uint),
                ("recovery_amount", C.c_float), ("recovery_percentage", C.c_float), ("visualize", C.c_int32)]


class AffineParams(C.Structure):
    _fields_ = [("mul", C.c_float), ("div", C.c_float), ("add", C.c_float), ("lo", C.c_float), ("hi", C.c_float),
                ("post_add", C.c_float)]


class AttentionParams(C.Structure):
    """silent_attention_params (include/silent_hip.h)."""
    _fields_ = [("region_h", C.c_int32), ("region_w", C.c_int32), ("resize_div", C.c_float), ("boosting", BoostingParams)]


class DisplayerParams(C.Structure):
    """silent_displayer_params (include/silent_hip.h)."""
    _fields_ = [("frame_h", C.c_int32), ("frame_w", C.c_int32), ("frame_dtype", C.c_int32), ("centroid_region_h", C.c_int32),
                ("centroid_region_w", C.c_int32), ("chain", RgbChainParams), ("boosting", BoostingParams)]


class FrameView(C.Structure):
    """silent_frame_view (include/silent_hip.h): strided uint8 frames, three BYTE strides."""
    _fields_ = [("data", C.c_void_p), ("channels", C.c_int), ("pixel_stride", C.c_int64), ("row_stride", C.c_int64),
                ("frame_stride", C.c_int64)]


class FrameView16(C.Structure):
    """silent_frame_view16 (include/silent_hip.h): strided uint16 frames, three BYTE strides (all even)."""
    _fields_ = [("data", C.c_void_p), ("pixel_stride", C.c_int64), ("row_stride", C.c_int64), ("frame_stride", C.c_int64)]


class Nv12Frames(C.Structure):
    """silent_nv12_frames (include/silent_hip.h): an NV12 batch -- luma plane, interleaved (U, V) plane, four BYTE strides, the 3 x 3
    conversion matrix (row k: output channel k) and the luma offset."""
    _fields_ = [("y", C.c_void_p), ("uv", C.c_void_p), ("y_row_stride", C.c_int64), ("y_frame_stride", C.c_int64),
                ("uv_row_stride", C.c_int64), ("uv_frame_stride", C.c_int64), ("m", C.c_float * 9), ("oy", C.c_float)]


class P010Frames(C.Structure):
    """silent_p010_frames (include/silent_hip.h): a P010 / P012 / P016 batch -- uint16 luma plane, interleaved (U, V) plane, four BYTE
    strides, the 3 x 3 conversion matrix (row k: output channel k), the luma and chroma offsets and shift = 16 - depth."""
    _fields_ = [("y", C.c_void_p), ("uv", C.c_void_p), ("y_row_stride", C.c_int64), ("y_frame_stride", C.c_int64),
                ("uv_row_stride", C.c_int64), ("uv_frame_stride", C.c_int64), ("m", C.c_float * 9), ("oy", C.c_float), ("oc", C.c_float),
                ("shift", C.c_int)]


class YuvFrames(C.Structure):
    """silent_yuv_frames (include/silent_hip.h): a planar / packed 8-bit YUV batch -- three plane pointers, the luma plane's pixel /
    row / frame strides and those the two chroma planes share (BYTES), the chroma shifts per axis, the 3 x 3 conversion matrix (row k:
    output channel k) and the luma offset."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("y_pixel_stride", C.c_int64), ("y_row_stride", C.c_int64), ("y_frame_stride", C.c_int64),
                ("c_pixel_stride", C.c_int64), ("c_row_stride", C.c_int64), ("c_frame_stride", C.c_int64),
                ("chroma_shift_x", C.c_int32), ("chroma_shift_y", C.c_int32), ("m", C.c_float * 9), ("oy", C.c_float)]


class Yuv16Frames(C.Structure):
    """silent_yuv16_frames (include/silent_hip.h): a planar / semi-planar / packed 16-bit YUV batch -- YuvFrames with uint16 elements
    (strides in BYTES, even), the chroma offset, and the position of the code value inside an element: shift bits below it, depth bits."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("y_pixel_stride", C.c_int64), ("y_row_stride", C.c_int64), ("y_frame_stride", C.c_int64),
                ("c_pixel_stride", C.c_int64), ("c_row_stride", C.c_int64), ("c_frame_stride", C.c_int64),
                ("chroma_shift_x", C.c_int32), ("chroma_shift_y", C.c_int32), ("m", C.c_float * 9), ("oy", C.c_float), ("oc", C.c_float),
                ("shift", C.c_int32), ("depth", C.c_int32)]


class BayerFrames(C.Structure):
    """silent_bayer_frames (include/silent_hip.h): a batch of raw 8-bit Bayer mosaics -- one byte plane, three BYTE strides, the pattern
    (0 .. 3: rggb, grbg, gbrg, bggr -- the top-left 2 x 2 cell of the view) and the channel order (0: bgr, 1: rgb)."""
    _fields_ = [("data", C.c_void_p), ("pixel_stride", C.c_int64), ("row_stride", C.c_int64), ("frame_stride", C.c_int64),
                ("pattern", C.c_int32), ("order", C.c_int32)]


class SilentLibraryError(RuntimeError):
    """libsilent_hip.so is missing or cannot be loaded."""


_lib = None

_vp = C.c_void_p
_fp = C.c_void_p          # float* passed as an address (host ndarray.ctypes.data or a device pointer)
_hp = C.POINTER(C.c_uint16)   # a float16 map (silent_gray_pass_h: IEEE binary16 as uint16_t*); half_ptr() makes one from an address
_bp = C.POINTER(C.c_uint8)    # uint8 frames (the *_u8, *_u8x3 and *_rgb8 entry points); byte_ptr() makes one from an address
_wp = C.POINTER(FrameView)    # a strided uint8 view (the *_view entry points); view_ptr() makes one from _runtime.frame_view_of's tuple
_sp = C.POINTER(C.c_uint16)   # uint16 frames (the *_u16 entry points); short_ptr() makes one from an address
_xp = C.POINTER(FrameView16)  # a strided uint16 view (the *_view16 entry points); view16_ptr() makes one from frame_view_of's tuple
_np = C.POINTER(Nv12Frames)   # an NV12 batch (silent_pyramid_nv12, silent_nv12_to_rgb); nv12_ptr() makes one from _runtime.nv12_frames_of's tuple
_pp = C.POINTER(P010Frames)   # a P010 batch (silent_pyramid_p010, silent_p010_to_rgb); p010_ptr() makes one from _runtime.p010_frames_of's tuple
_yp = C.POINTER(YuvFrames)    # a planar / packed YUV batch (silent_pyramid_yuv, silent_yuv_to_rgb); yuv_ptr() makes one from _runtime.yuv_frames_of's tuple
_y16p = C.POINTER(Yuv16Frames)  # a 16-bit YUV batch (silent_pyramid_yuv16, silent_yuv16_to_rgb); yuv16_ptr() makes one from _runtime.yuv16_frames_of's tuple
_byp = C.POINTER(BayerFrames)   # a batch of Bayer mosaics (silent_pyramid_bayer, silent_bayer_to_rgb); bayer_ptr() makes one from _runtime.bayer_frames_of's tuple
_ep = C.POINTER(Extent)
_i, _u, _f, _d, _sz = C.c_int, C.c_uint, C.c_float, C.c_double, C.c_size_t

# name -> argtypes (restype is int unless listed in _RESTYPES)
_SIGNATURES = {
    "silent_abi_version": [],
    "silent_device_count": [C.POINTER(_i)],
    "silent_create": [_i, C.POINTER(_vp)],
    "silent_destroy": [_vp],
    "silent_last_error": [_vp],
    "silent_device_name": [_vp, C.c_char_p, _sz],
    "silent_malloc": [_vp, _sz, C.POINTER(_vp)],
    "silent_free": [_vp, _vp],
    "silent_memcpy_h2d": [_vp, _vp, _vp, _sz, _vp],
    "silent_memcpy_d2h": [_vp, _vp, _vp, _sz, _vp],
    "silent_synchronize": [_vp, _vp],
    "silent_busy_wait_dev": [_vp, _u, _vp],
    "silent_trace_marker_dev": [_vp, _vp],
    "silent_pyramid_plan_create": [_vp, _i, _i, _i, C.POINTER(PyrLevel), _i, C.POINTER(_vp)],
    "silent_pyramid_plan_create_ex": [_vp, _i, _i, _i, C.POINTER(PyrLevel), _i, _u, C.POINTER(_vp)],
    "silent_pyramid_plan_flags": [_vp, C.POINTER(C.c_uint)],
    "silent_pyramid_plan_destroy": [_vp],
    "silent_pyramid": [_vp, _vp, _fp, _i, _fp],
    "silent_pyramid_dev": [_vp, _vp, _fp, _i, _fp, _vp],
    "silent_conv2d_same": [_vp, _fp, _ep, _i, _i, _i, _fp, _i, _i, _i, _u, _f, _fp],
    "silent_conv2d_same_dev": [_vp, _fp, _ep, _i, _i, _i, _fp, _i, _i, _i, _u, _f, _fp, _vp],
    "silent_gray_line_end": [_vp, _fp, _ep, _i, _i, _fp, _fp, _i, _f, _fp, _fp],
    "silent_gray_line_end_dev": [_vp, _fp, _ep, _i, _i, _fp, _fp, _i, _f, _fp, _fp, _vp],
    "silent_gray_pass": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp],
    "silent_gray_pass_dev": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _vp],
    "silent_gray_pass_parts_dev": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _u, _vp],
    "silent_gray_pass_h": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _hp, _hp],
    "silent_gray_pass_h_dev": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _hp, _hp, _u, _vp],
    "silent_pyramid_u8": [_vp, _vp, _bp, _i, _fp],
    "silent_pyramid_u8x3": [_vp, _vp, _bp, _i, _fp],
    "silent_pyramid_u8_dev": [_vp, _vp, _bp, _i, _fp, _vp],
    "silent_pyramid_u8x3_dev": [_vp, _vp, _bp, _i, _fp, _vp],
    "silent_pyramid_rgb8": [_vp, _vp, _bp, _i, _fp],
    "silent_pyramid_rgb8_dev": [_vp, _vp, _bp, _i, _fp, _vp],
    "silent_pyramid_rgb8_view": [_vp, _vp, _wp, _i, _fp],
    "silent_pyramid_rgb8_view_dev": [_vp, _vp, _wp, _i, _fp, _vp],
    "silent_pyramid_nv12": [_vp, _vp, _np, _i, _fp],
    "silent_pyramid_nv12_dev": [_vp, _vp, _np, _i, _fp, _vp],
    "silent_nv12_to_rgb": [_vp, _np, _i, _i, _i, _fp],
    "silent_nv12_to_rgb_dev": [_vp, _np, _i, _i, _i, _fp, _vp],
    "silent_pyramid_p010": [_vp, _vp, _pp, _i, _fp],
    "silent_pyramid_p010_dev": [_vp, _vp, _pp, _i, _fp, _vp],
    "silent_p010_to_rgb": [_vp, _pp, _i, _i, _i, _fp],
    "silent_p010_to_rgb_dev": [_vp, _pp, _i, _i, _i, _fp, _vp],
    "silent_pyramid_yuv": [_vp, _vp, _yp, _i, _fp],
    "silent_pyramid_yuv_dev": [_vp, _vp, _yp, _i, _fp, _vp],
    "silent_yuv_to_rgb": [_vp, _yp, _i, _i, _i, _fp],
    "silent_yuv_to_rgb_dev": [_vp, _yp, _i, _i, _i, _fp, _vp],
    "silent_pyramid_yuv16": [_vp, _vp, _y16p, _i, _fp],
    "silent_pyramid_yuv16_dev": [_vp, _vp, _y16p, _i, _fp, _vp],
    "silent_yuv16_to_rgb": [_vp, _y16p, _i, _i, _i, _fp],
    "silent_yuv16_to_rgb_dev": [_vp, _y16p, _i, _i, _i, _fp, _vp],
    "silent_pyramid_bayer": [_vp, _vp, _byp, _i, _fp],
    "silent_pyramid_bayer_dev": [_vp, _vp, _byp, _i, _fp, _vp],
    "silent_bayer_to_rgb": [_vp, _byp, _i, _i, _i, _fp],
    "silent_bayer_to_rgb_dev": [_vp, _byp, _i, _i, _i, _fp, _vp],
    "silent_gray_pass_u8": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i],
    "silent_gray_pass_u8x3": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i],
    "silent_gray_pass_u8_dev": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i, _u, _vp],
    "silent_gray_pass_u8x3_dev": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i, _u, _vp],
    "silent_pyramid_view": [_vp, _vp, _wp, _i, _fp],
    "silent_pyramid_view_dev": [_vp, _vp, _wp, _i, _fp, _vp],
    "silent_gray_pass_view": [_vp, _vp, _wp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i],
    "silent_gray_pass_view_dev": [_vp, _vp, _wp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i, _u, _vp],
    "silent_pyramid_u16": [_vp, _vp, _sp, _i, _fp],
    "silent_pyramid_u16_dev": [_vp, _vp, _sp, _i, _fp, _vp],
    "silent_gray_pass_u16": [_vp, _vp, _sp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i],
    "silent_gray_pass_u16_dev": [_vp, _vp, _sp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i, _u, _vp],
    "silent_pyramid_view16": [_vp, _vp, _xp, _i, _fp],
    "silent_pyramid_view16_dev": [_vp, _vp, _xp, _i, _fp, _vp],
    "silent_gray_pass_view16": [_vp, _vp, _xp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i],
    "silent_gray_pass_view16_dev": [_vp, _vp, _xp, _i, _fp, _fp, _i, _f, _fp, _vp, _vp, _i, _u, _vp],
    "silent_pyramid_plan_is_streamable": [_vp],
    "silent_pyramid_plan_walk_plans": [_vp, C.POINTER(C.c_int)],
    "silent_gather_d2h": [_vp, _vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), _i, _vp],
    "silent_set_profiling": [_vp, _i],
    "silent_set_tuning": [_vp, _i, _u],
    "silent_get_tuning": [_vp, _i, C.POINTER(C.c_uint)],
    "silent_profile_elapsed_ms": [_vp, C.POINTER(_f), C.POINTER(C.c_int64)],
    "silent_regulate": [_vp, _fp, _ep, _i, _i, _i, _fp, _i, _i, _f, _f, _i, _fp],
    "silent_regulate_dev": [_vp, _fp, _ep, _i, _i, _i, _fp, _i, _i, _f, _f, _i, _fp, _vp],
    "silent_pad_inwards": [_vp, _fp, _ep, _i, _i, _i, _i, _i, _i, _i, _fp],
    "silent_pad_inwards_dev": [_vp, _fp, _ep, _i, _i, _i, _i, _i, _i, _i, _fp, _vp],
    "silent_value_from_color": [_vp, _fp, _ep, _i, _i, _i, _fp],
    "silent_value_from_color_dev": [_vp, _fp, _ep, _i, _i, _i, _fp, _vp],
    "silent_bw_from_color": [_vp, _fp, _ep, _i, _i, _i, _fp],
    "silent_bw_from_color_dev": [_vp, _fp, _ep, _i, _i, _i, _fp, _vp],
    "silent_nms3x3": [_vp, _fp, _ep, _i, _i, _i, _i, _fp],
    "silent_nms3x3_dev": [_vp, _fp, _ep, _i, _i, _i, _i, _fp, _vp],
    "silent_top_value_points": [_vp, _fp, _fp, _ep, _i, _i, _i, _d, _fp],
    "silent_top_value_points_dev": [_vp, _fp, _fp, _ep, _i, _i, _i, _d, _fp, _vp],
    "silent_max_value_indices_region": [_vp, _fp, _ep, _i, _i, _ep, _vp, _sz, _vp],
    "silent_max_value_indices_region_dev": [_vp, _fp, _ep, _i, _i, _ep, _vp, _sz, _vp, _vp],
    "silent_select_peaks": [_vp, _fp, _fp, _ep, _i, _i, _i, _d, _fp, _fp, _fp],
    "silent_select_peaks_dev": [_vp, _fp, _fp, _ep, _i, _i, _i, _d, _fp, _fp, _fp, _vp],
    "silent_select_keypoints": [_vp, _fp, _fp, _ep, _i, _i, _i, _d, _ep, _fp, _vp, _sz, _vp],
    "silent_select_keypoints_dev": [_vp, _fp, _fp, _ep, _i, _i, _i, _d, _ep, _fp, _vp, _sz, _vp, _vp],
    "silent_centroids": [_vp, _fp, _ep, _i, _i, _i, _i, _fp, _fp],
    "silent_centroids_dev": [_vp, _fp, _ep, _i, _i, _i, _i, _fp, _fp, _vp],
    "silent_boosting_step": [_vp, _fp, _ep, _i, _i, C.POINTER(BoostingParams), _fp, _fp, _fp],
    "silent_boosting_step_dev": [_vp, _fp, _ep, _i, _i, C.POINTER(BoostingParams), _fp, _fp, _fp, _vp],
    "silent_affine_clip": [_vp, _fp, _sz, C.POINTER(AffineParams), _fp],
    "silent_affine_clip_dev": [_vp, _fp, _sz, C.POINTER(AffineParams), _fp, _vp],
    "silent_cast_interleave": [_vp, _vp, _i, _sz, _i, _i, _i, _fp, _i, _i],
    "silent_cast_interleave_dev": [_vp, _vp, _i, _sz, _i, _i, _i, _fp, _i, _i, _vp],
    "silent_resize_nearest": [_vp, _fp, _ep, _i, _i, _i, _ep, _fp],
    "silent_resize_nearest_dev": [_vp, _fp, _ep, _i, _i, _i, _ep, _fp, _vp],
    "silent_rgb_chain_structure": [C.POINTER(RgbChainParams), C.POINTER(C.c_uint), C.POINTER(C.c_uint)],
    "silent_rgb_keypoints": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _d, _ep, _fp, _fp, _fp, _fp, _vp, _sz, _vp],
    "silent_rgb_keypoints_dev": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _d, _ep, _fp, _fp, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_rgb_keypoints_h": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _d, _ep, _hp, _hp, _fp, _fp, _vp, _sz, _vp],
    "silent_rgb_keypoints_h_dev": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _d, _ep, _hp, _hp, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_gray_keypoints": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp],
    "silent_gray_keypoints_dev": [_vp, _vp, _fp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_gray_keypoints_u8": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp],
    "silent_gray_keypoints_u8x3": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp],
    "silent_gray_keypoints_u8_dev": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_gray_keypoints_u8x3_dev": [_vp, _vp, _bp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_gray_keypoints_view": [_vp, _vp, _wp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp],
    "silent_gray_keypoints_view_dev": [_vp, _vp, _wp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_gray_keypoints_u16": [_vp, _vp, _sp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp],
    "silent_gray_keypoints_u16_dev": [_vp, _vp, _sp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_gray_keypoints_view16": [_vp, _vp, _xp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp],
    "silent_gray_keypoints_view16_dev": [_vp, _vp, _xp, _i, _fp, _fp, _i, _f, _fp, _fp, _fp, _i, _i, _d, _ep, _fp, _fp, _vp, _sz, _vp, _vp],
    "silent_sparse_tail_stats": [_vp, C.POINTER(C.c_int64)],
    "silent_rgb_chain_stream": [C.POINTER(RgbChainParams), C.c_uint, _fp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "silent_rgb_line_end": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _fp, _fp, _fp],
    "silent_rgb_line_end_dev": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _fp, _fp, _fp, _vp],
    "silent_rgb_line_end_h": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _hp, _hp, _fp],
    "silent_rgb_line_end_h_dev": [_vp, _fp, _ep, _i, _i, C.POINTER(RgbChainParams), _hp, _hp, _fp, _vp],
    "silent_displayer_create": [_vp, C.POINTER(DisplayerParams), C.POINTER(PyrLevel), _i, C.POINTER(_vp)],
    "silent_displayer_destroy": [_vp],
    "silent_displayer_shape": [_vp, C.POINTER(C.c_int32), C.POINTER(_sz)],
    "silent_displayer_step": [_vp, _vp, C.POINTER(_vp), C.POINTER(_f)],
    "silent_displayer_add_slot": [_vp, C.POINTER(_i)],
    "silent_displayer_step_slot": [_vp, _vp, _i, C.POINTER(_vp), C.POINTER(_f)],
    "silent_displayer_input": [_vp, C.POINTER(_vp), C.POINTER(_sz)],
    "silent_displayer_get_state": [_vp, _fp],
    "silent_displayer_set_state": [_vp, _fp],
    "silent_attention_extents": [_ep, _i, C.POINTER(AttentionParams), _ep, _ep, _ep],
    "silent_attention_tail": [_vp, _fp, _ep, _i, _i, C.POINTER(AttentionParams), _fp, _fp, _fp, _fp, _fp],
    "silent_attention_tail_dev": [_vp, _fp, _ep, _i, _i, C.POINTER(AttentionParams), _fp, _fp, _fp, _fp, _fp, _vp],
}
_RESTYPES = {"silent_destroy": None, "silent_pyramid_plan_destroy": None, "silent_displayer_destroy": None, "silent_last_error": C.c_char_p}

EXPORTED_SYMBOLS = tuple(sorted(_SIGNATURES))


def half_ptr(address):
    """A host or device address as the uint16_t* of a float16 map argument (None: NULL)."""
    return None if address is None else C.cast(C.c_void_p(int(address)), _hp)


def byte_ptr(address):
    """A host or device address as the const uint8_t* of a uint8 frames argument (None: NULL)."""
    return None if address is None else C.cast(C.c_void_p(int(address)), _bp)


def short_ptr(address):
    """A host or device address as the const uint16_t* of a uint16 frames argument (None: NULL)."""
    return None if address is None else C.cast(C.c_void_p(int(address)), _sp)


def void_ptr(address):
    """A host or device address as a void* / float* argument (None: NULL)."""
    return None if address is None else C.c_void_p(int(address))


def view_ptr(view):
    """(address, channels, pixel_stride, row_stride, frame_stride) -- what _runtime.frame_view_of returns -- as the
    const silent_frame_view* of a *_view entry point (None: NULL).  The struct is read before the call returns."""
    if view is None:
        return None
    address, channels, pixel_stride, row_stride, frame_stride = view
    return C.pointer(FrameView(int(address), int(channels), int(pixel_stride), int(row_stride), int(frame_stride)))


def view16_ptr(view):
    """The same tuple for a uint16 view (its channels entry is 1) as the const silent_frame_view16* of a *_view16 entry point."""
    if view is None:
        return None
    address, _channels, pixel_stride, row_stride, frame_stride = view
    return C.pointer(FrameView16(int(address), int(pixel_stride), int(row_stride), int(frame_stride)))


def struct_ptr(struct, fields):
    """A tuple of the fields of ``struct`` in their order (an array member, the c_float * 9 matrix, as a sequence) as a pointer to the
    struct (None: NULL).  The struct is read before the call returns."""
    if fields is None:
        return None
    if len(fields) != len(struct._fields_):
        raise ValueError("%s takes %d fields, got %d" % (struct.__name__, len(struct._fields_), len(fields)))
    return C.pointer(struct(*[t(*[float(c) for c in v]) if issubclass(t, C.Array) else (float(v) if t is C.c_float else int(v))
                              for (_, t), v in zip(struct._fields_, fields)]))


def nv12_ptr(frames):
    """_runtime.nv12_frames_of's tuple as the const silent_nv12_frames* of the NV12 entry points."""
    return struct_ptr(Nv12Frames, frames)


def p010_ptr(frames):
    """_runtime.p010_frames_of's tuple as the const silent_p010_frames* of the P010 entry points."""
    return struct_ptr(P010Frames, frames)


def yuv_ptr(frames):
    """_runtime.yuv_frames_of's tuple as the const silent_yuv_frames* of the YUV entry points."""
    return struct_ptr(YuvFrames, frames)


def yuv16_ptr(frames):
    """_runtime.yuv16_frames_of's tuple as the const silent_yuv16_frames* of the 16-bit YUV entry points."""
    return struct_ptr(Yuv16Frames, frames)


def bayer_ptr(frames):
    """_runtime.bayer_frames_of's tuple as the const silent_bayer_frames* of the Bayer entry points."""
    return struct_ptr(BayerFrames, frames)


def gray_entry(family, frame_dtype="float32", frame_channels=1, storage="float32", dev=False, parts=None, frame_layout="packed"):
    """The call shape of the gray pass ("gray_pass") or its keypoint form ("gray_keypoints") for a frame layout, a map storage and the
    host or _dev form: (name, frame_ptr, map_ptr, tail) -- the entry point silent_<name>[_dev], what makes its frames argument and its
    cs_out / end_out arguments from an address, and the arguments that follow end_out (maps_f16, parts) before the stream.  parts:
    None = the whole pass; 1 / 2 / 3 = the halves of an overlapped step (_dev forms).  frame_layout="strided" (uint8 / uint16 frames): the
    *_view / *_view16 entry points, whose frames argument view_ptr / view16_ptr makes from a view tuple (_runtime.frame_view_of), not
    from an address.  frame_dtype="uint16": the *_u16 / *_view16 entry points (one channel)."""
    if frame_dtype == "uint16":
        sfx = "_view16" if frame_layout == "strided" else "_u16"
    else:
        sfx = "" if frame_dtype != "uint8" else "_view" if frame_layout == "strided" else "_u8x3" if frame_channels == 3 else "_u8"
    frame_ptr = view_ptr if sfx == "_view" else view16_ptr if sfx == "_view16" else short_ptr if sfx == "_u16" else byte_ptr if sfx else void_ptr
    if family != "gray_pass":
        return family + sfx, frame_ptr, void_ptr, ()
    parts_arg = (3 if parts is None else int(parts),) if dev else ()
    if sfx:
        return family + sfx, frame_ptr, void_ptr, (int(storage == "float16"),) + parts_arg
    if storage == "float16":
        return family + "_h", frame_ptr, half_ptr, parts_arg
    if dev and parts is not None:
        return family + "_parts", frame_ptr, void_ptr, parts_arg
    return family, frame_ptr, void_ptr, ()


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so with the same
    SONAME as /opt/rocm's; if torch is installed, load ITS copy first (by path, RTLD_GLOBAL) so that our
    DT_NEEDED libamdhip64.so.7 binds to the very file ``import torch`` will map later.  Without torch the
    library's RUNPATH (/opt/rocm/lib) applies."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load (once) and return the ctypes handle; raises SilentLibraryError when the .so is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SilentLibraryError(
            "%s not found: build it with `python pysilent_amd/csrc/build.py` (hipcc --offload-arch=gfx950). "
            "pysilent_amd has no CPU fallback." % LIB_PATH)
    _preload_hip_runtime()
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise SilentLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, C.c_int)
    got = lib.silent_abi_version()
    if got != ABI_VERSION:
        raise SilentLibraryError("libsilent_hip.so ABI %d != binding ABI %d" % (got, ABI_VERSION))
    _lib = lib
    return lib


def last_error(ctx_handle):
    msg = load().silent_last_error(ctx_handle)
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, ctx_handle=None):
    """Map a silent_status to the Python exception the reference's callers would see."""
    if rc == SILENT_OK:
        return
    msg = last_error(ctx_handle) or ("silent_status %d" % rc)
    if rc in (SILENT_E_INVALID, SILENT_E_UNSUPPORTED, SILENT_E_CAPACITY):
        raise ValueError(msg)
    if rc == SILENT_E_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)
