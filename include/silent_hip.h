/* silent_hip.h -- C ABI of libsilent_hip.so: the MI355X (gfx950) implementation of pySILEnT's
 * scale-space center-surround / oriented line-end detector hot path.
 *
 * The reference (SimLeek/pySILEnT, /root/reference) has NO plugin / operator / FFI layer: its
 * boundary is a set of plain Python functions that build TensorFlow-1.x graph nodes
 * (SURVEY.md section 8b).  Each entry point below therefore cites the reference *function* it
 * replaces (path:line relative to /root/reference); the Python binding a maintainer would add
 * (ctypes) is shown in INTEGRATION.md and implemented in pysilent_amd/_lib.py.
 *
 * Conventions
 *   - Activations: float32, NHWC, "packed pyramid batch": n_frames consecutive pyramids, each
 *     pyramid = level 0 .. level n_levels-1 back to back, level l = h_l x w_l x C row-major.
 *     The reference's fixed-size layout [L, h, w, C] (util/zoom/from_image.py:47) is the special
 *     case n_frames = 1, all extents equal -- byte-identical to the NumPy array it feeds TF.
 *   - Kernels: float32, HWIO [kh, kw, C_in, C_out] (what tf.constant(k, dtype=tf.float32) holds).
 *   - Convolutions: stride 1, SAME zero padding (pad_before = (k-1)/2), cross-correlation.
 *   - Every function returns SILENT_OK (0) or a negative silent_status; the message is available
 *     from silent_last_error().  Nothing throws or aborts across the ABI.
 *   - Ownership: the caller owns every buffer; the library never keeps a caller pointer past
 *     return.  silent_ctx / silent_pyramid_plan are library-owned handles.
 *   - Threading: a silent_ctx is not thread-safe; use one per (host thread, GPU).  Several entry points keep
 *     temporaries (reduction slots, chunk counts, staged intermediates) in ONE workspace owned by the context.  The
 *     library enforces the ordering this needs: when a workspace-using *_dev call arrives on another stream than the
 *     previous one, that previous stream is drained first (correct, but serialising: streams that should overlap need
 *     a context each).  The entry points run on the context's device and restore the caller's current HIP device.
 *   - Entry points without suffix take HOST pointers and are synchronous (they stage through the
 *     context's device arena).  The *_dev twins take DEVICE pointers plus a hipStream_t (passed as
 *     void*; NULL = the legacy default stream), are stream-ordered and do not synchronise.
 */
#ifndef SILENT_HIP_H
#define SILENT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SILENT_ABI_VERSION 5
#define SILENT_MAX_LEVELS 16
#define SILENT_MAX_KERNEL_FLOATS 784 /* kh*kw*C_in*C_out limit (weights travel as kernel arguments) */

typedef enum silent_status {
    SILENT_OK = 0,
    SILENT_E_INVALID = -1,     /* bad argument (NULL pointer, extent <= 0, channel mismatch ...)  -> ValueError */
    SILENT_E_HIP = -2,         /* a HIP runtime call failed                                       -> RuntimeError */
    SILENT_E_CAPACITY = -3,    /* caller-provided index buffer too small; counts hold the need    -> ValueError */
    SILENT_E_UNSUPPORTED = -4, /* shape outside the compiled set                                  -> ValueError */
    SILENT_E_NOMEM = -5        /* device allocation failed                                        -> MemoryError */
} silent_status;

typedef struct silent_ctx silent_ctx;
typedef struct silent_pyramid_plan silent_pyramid_plan;
typedef void* silent_stream; /* hipStream_t */

typedef struct silent_extent {
    int32_t h, w;
} silent_extent;

/* conv flags */
#define SILENT_RELU 1u /* tf.maximum(x, [0])            filters/rgc.py:13-16 */
#define SILENT_CLIP 2u /* tf.clip_by_value(x, 0, hi)    recognition_testing.py:74 */

/* regulate_tensor flat-region policy (hard part 3) */
#define SILENT_FLAT_IEEE 0 /* literal: 0 * (rv / pow(0, root)) = NaN */
#define SILENT_FLAT_ZERO 1 /* output 0 where the input is exactly 0 */

/* nms modes */
#define SILENT_NMS_PRODUCT 0 /* x * where(x == maxpool3x3(x), x, 0)   _experimental/vision_filter.py:88-89 */
#define SILENT_NMS_FIRED 1   /* where(x == maxpool3x3(x), 1, 0)       util/energy/boosting.py:18-22 */

/* ---------------------------------------------------------------------------- context */

int silent_abi_version(void);
/* Number of HIP devices visible (0 and SILENT_E_HIP when the runtime cannot initialise). */
int silent_device_count(int* count);
int silent_create(int device, silent_ctx** out);
void silent_destroy(silent_ctx* ctx);
/* Last error text of this context; ctx may be NULL (then: the last error of a failed silent_create). */
const char* silent_last_error(const silent_ctx* ctx);
int silent_device_name(const silent_ctx* ctx, char* buf, size_t len);

/* Device-memory helpers so that a host without PyTorch can stay device-resident. */
int silent_malloc(silent_ctx* ctx, size_t bytes, void** dptr);
int silent_free(silent_ctx* ctx, void* dptr);
int silent_memcpy_h2d(silent_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, silent_stream stream);
int silent_memcpy_d2h(silent_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, silent_stream stream);
/* n device buffers -> ONE host buffer, back to back, with a single synchronisation at the end: the fetch of
 * session.run([t0 .. t5]) (slam_recognition/recognition_testing.py:132) for results that live on the device. */
int silent_gather_d2h(silent_ctx* ctx, void* dst_host, const void* const* src_dev, const size_t* bytes, int n,
                      silent_stream stream);
int silent_synchronize(silent_ctx* ctx, silent_stream stream);
/* Occupies `stream` for about `microseconds` (one wavefront polling the constant-rate clock; <= 1 s): the probe a host
 * uses to find out whether two streams really run side by side (pysilent_amd.pipeline.pick_concurrent_stream).  No
 * counterpart in the reference (it has one stream: tf.device('/device:GPU:0'), recognition_testing.py:64). */
int silent_busy_wait_dev(silent_ctx* ctx, unsigned microseconds, silent_stream stream);
/* One empty kernel named trace_marker_kernel on `stream`: a mark in a rocprofv3 kernel trace (bench.py puts it between its tuners
 * and the measured steps; scripts/summarize_profile.py reads the statistics behind it).  No counterpart in the reference. */
int silent_trace_marker_dev(silent_ctx* ctx, silent_stream stream);

/* ---------------------------------------------------------------------------- a-1 pyramid
 * Replaces image_to_zoom_tensor, slam_recognition/util/zoom/from_image.py:10-69: per level a crop of
 * the frame resampled by scipy.ndimage.zoom(plane, z, prefilter=False, order=5) (from_image.py:55-59:
 * un-prefiltered quintic B-spline, output o -> o*(in-1)/(out-1), mirror tap extension, mode
 * 'constant' out-of-range rule) and copied to the top-left of a canvas (from_image.py:61-64).
 * Canvas pixels the zoomed crop does not cover are uninitialised in the reference; here they are 0.
 * The HOST decides crop and zoom extents (Python's round() is part of scipy's contract) and passes
 * them explicitly; "classic" whole-frame levels are the case crop = frame, out = zoom extents. */
typedef struct silent_pyr_level {
    int32_t src_y0, src_x0, src_h, src_w; /* crop of the frame that the resampler sees        */
    int32_t zoom_h, zoom_w;               /* resampler output extents = round(src * zoom)     */
    int32_t out_h, out_w;                 /* canvas (level) extents; copied region = min(zoom, out) */
} silent_pyr_level;

int silent_pyramid_plan_create(silent_ctx* ctx, int frame_h, int frame_w, int channels,
                               const silent_pyr_level* levels, int n_levels, silent_pyramid_plan** out);
/* silent_pyramid_plan_create with flags (silent_pyramid_plan_create is this call with flags = 0).
 * SILENT_PLAN_ACCUM_F64: float64 accumulation inside each op, like the CPU oracle.  Every map is still stored as float32; within
 * one op the taps are summed in float64 and rounded to float32 once: the 6 x 6 spline taps of a pyramid output (float64 weights,
 * vertical and horizontal sums, so a stored value may differ from the oracle's 2-D sum by 1 ulp where the double rounding lands
 * near a midpoint), the 9 CS taps, the 9 * K end taps (in the oracle's order: the CS and end maps of a given pyramid are
 * bit-identical to it).  Single-channel plans only (channels = 3: SILENT_E_UNSUPPORTED); unknown bits: SILENT_E_INVALID.
 * Honoured by silent_pyramid[_dev], silent_gray_pass[_dev], silent_gray_pass_parts_dev and silent_gray_keypoints[_dev]; the
 * per-op silent_gray_line_end[_dev] takes no plan and always accumulates in float32. */
#define SILENT_PLAN_ACCUM_F64 1u
int silent_pyramid_plan_create_ex(silent_ctx* ctx, int frame_h, int frame_w, int channels, const silent_pyr_level* levels,
                                  int n_levels, unsigned flags, silent_pyramid_plan** out);
/* The flags the plan was created with. */
int silent_pyramid_plan_flags(const silent_pyramid_plan* plan, unsigned* flags);
void silent_pyramid_plan_destroy(silent_pyramid_plan* plan);
/* frames: n_frames x [H, W, C] float32 (values as the reference feeds them: uint8 range cast to f32,
 * recognition_testing.py:141).  pyr: packed pyramid batch with the plan's canvas extents. */
int silent_pyramid(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames, float* pyr);
int silent_pyramid_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                       float* pyr, silent_stream stream);

/* ---------------------------------------------------------------------------- a-2..a-5 convolution
 * Replaces the tf.nn.conv2d(+tf.maximum(+tf.clip_by_value)) call sites:
 *   rgc_filter          slam_recognition/filters/rgc.py:6-18
 *   rgby_filter         slam_recognition/filters/rgby.py:6-14
 *   orientation_filter  slam_recognition/filters/orientation.py:17-29 (the stripe conv)
 *   apply_filter        slam_recognition/util/apply_filter.py:4-7 (+ relu/clip recognition_testing.py:73-74)
 * flags: SILENT_RELU | SILENT_CLIP (clip to [0, clip_hi]); NaN handling is Eigen's (x < 0 ? 0 : x). */
int silent_conv2d_same(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                       int c_in, const float* kernel_hwio, int kh, int kw, int c_out, unsigned flags,
                       float clip_hi, float* out);
int silent_conv2d_same_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                           int n_frames, int c_in, const float* kernel_hwio, int kh, int kw, int c_out,
                           unsigned flags, float clip_hi, float* out, silent_stream stream);

/* ---------------------------------------------------------------------------- fused grayscale pass
 * BASELINE configs 1/2/5: per level
 *     cs  = relu(conv3x3(x,  cs_kernel[3,3,1,1]))
 *     end = clip(relu(conv3x3(cs, end_bank[3,3,1,K])), 0, clip_hi)
 * i.e. the reference chain order recognition_testing.py:69-74 restricted to one input channel, in one
 * kernel launch (the CS map never leaves LDS between the two convolutions).  K in {3, 4, 8}.
 * cs_out: packed [.., h_l, w_l, 1]; end_out: packed [.., h_l, w_l, K]; either may be NULL to skip it. */
int silent_gray_line_end(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                         const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi,
                         float* cs_out, float* end_out);
int silent_gray_line_end_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                             int n_frames, const float* cs_kernel, const float* end_bank, int n_orient,
                             float clip_hi, float* cs_out, float* end_out, silent_stream stream);

/* ---------------------------------------------------------------------------- whole grayscale hot path
 * frames -> zoom pyramid -> CS -> ReLU -> K-orientation end bank -> ReLU -> clip in ONE call: the op order of
 * LineEndDisplayer.callback + compile (recognition_testing.py:136-144, :69-74) restricted to one channel.
 * Results are identical to silent_pyramid_dev followed by silent_gray_line_end_dev; the difference is traffic:
 * levels whose zoom factor is exactly 1 (level 0, 75 % of the pixels) are smoothed, center-surround filtered
 * and line-end filtered in one kernel, so that level is written once and never re-read.
 * pyr / cs_out / end_out: packed pyramid batches with the plan's extents (1, 1 and K channels); pyr is
 * always written (it is an output of the reference's from_image); cs_out or end_out may be NULL. */
int silent_gray_pass(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                     const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                     float* cs_out, float* end_out);
int silent_gray_pass_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                         const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                         float* cs_out, float* end_out, silent_stream stream);
/* The same pass in two halves, for callers that overlap consecutive batches on two streams (the reference runs one frame per
 * session.run, recognition_testing.py:132; a batched caller can run the second half of batch n beside the first half of batch
 * n + 1).  parts bit 0 (SILENT_GRAY_PART_PYRAMID): the pyramid of every level + CS / end of the unit-zoom levels -- reads
 * frames, writes pyr and the unit levels of cs_out / end_out; bit 1 (SILENT_GRAY_PART_FILTER): CS + end of the remaining
 * levels -- reads pyr (as written by part 0 for the same frames), writes the other levels of cs_out / end_out.  parts = 3 is
 * silent_gray_pass_dev.  The two parts of one batch must be ordered by the caller (same stream, or an event). */
#define SILENT_GRAY_PART_PYRAMID 1u
#define SILENT_GRAY_PART_FILTER 2u
int silent_gray_pass_parts_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                               const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                               float* cs_out, float* end_out, unsigned parts, silent_stream stream);

/* float16 storage of the CS and end maps: the pass above (same op order, recognition_testing.py:136-144, :69-74) with cs_out and
 * end_out stored as IEEE binary16 -- half the bytes of the two maps a caller keeps (their consumers are a display path that divides
 * by 255, recognition_testing.py:54, :79, and a selection that reads values in [0, clip_hi]).  Every stored element is float16(v),
 * v being the float32 value silent_gray_pass[_dev] stores for that element: all arithmetic is the float32 code, the conversion
 * happens at the store, round-to-nearest-even, overflow to +-inf, NaN stays NaN (sign and payload unspecified), subnormals kept.
 * pyr stays float32 (an output of the reference's from_image, and the filter of the non-unit levels reads it back).  end_out keeps
 * its NHWC layout [.., h, w, K], 2 * K bytes per pixel; end_out must be 16-byte and cs_out 2-byte aligned.  cs_out or end_out may
 * be NULL.  parts as silent_gray_pass_parts_dev (3 = the whole pass).  SILENT_E_UNSUPPORTED: a 3-channel plan, a plan created
 * with SILENT_PLAN_ACCUM_F64, n_orient other than 3, 4 or 8.  There is no float16 form of silent_gray_keypoints (its tail reads
 * the end map as float32) nor of the per-op silent_gray_line_end. */
int silent_gray_pass_h(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                       const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                       uint16_t* cs_out, uint16_t* end_out);
int silent_gray_pass_h_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                           const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                           uint16_t* cs_out, uint16_t* end_out, unsigned parts, silent_stream stream);

/* uint8 frames, read as they are.  Every real source of frames delivers uint8 (a camera, a decoder; the reference widens with
 * np.asarray(frame, float32), recognition_testing.py:141); these entry points take them without a widening cast and without a
 * float32 copy of the batch.  frames: [n_frames, H, W] bytes (one channel), NO alignment requirement.  The frame-reading kernels
 * load the byte and convert it in a register -- uint8 -> float32 is exact -- so every output is IDENTICAL, bit for bit, to that of
 * the float32-frame entry point given (float)frames[i]: silent_pyramid[_dev], silent_gray_pass_parts_dev (maps_f16 = 0),
 * silent_gray_pass_h_dev (maps_f16 = 1: cs_out / end_out are binary16 maps with silent_gray_pass_h's alignment rules) and
 * silent_gray_keypoints[_dev].  parts as silent_gray_pass_parts_dev.  The host-pointer forms stage H * W * n_frames BYTES of frames.
 * Status codes as silent_gray_pass_h: SILENT_E_INVALID for a NULL plan / frames / pyr, both outputs NULL, n_frames < 1, parts = 0,
 * a plan of another context; SILENT_E_UNSUPPORTED for a 3-channel plan, a SILENT_PLAN_ACCUM_F64 plan, n_orient other than 3, 4, 8.
 * (Not a plan flag: one plan serves both kinds of frames.  ABI additions only: SILENT_ABI_VERSION is unchanged.) */
int silent_pyramid_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, float* pyr);
int silent_pyramid_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, float* pyr,
                          silent_stream stream);
int silent_gray_pass_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                        const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                        void* end_out, int maps_f16);
int silent_gray_pass_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                            const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                            void* end_out, int maps_f16, unsigned parts, silent_stream stream);

/* Interleaved 3-channel uint8 frames, read as they are: what a camera or decoder hands over is colour, [H, W, 3] uint8 (the reference's
 * callback receives exactly that, BGR from OpenCV: recognition_testing.py:141) and the reference's colour-to-one-channel op is
 * get_value_from_color (util/color/get_value.py:6-12; silent_value_from_color, a-8).  These entry points are the twins of the *_u8 ones
 * above -- same argument lists, parts / maps_f16 / stream arguments and status codes -- for frames: [n_frames, H, W, 3] bytes, NO
 * alignment requirement.  The plan is a SINGLE-CHANNEL plan (it describes the pyramid; the frame layout is a property of the call).
 * Each frame pixel enters the arithmetic as
 *     v = (float)(b0 + b1 + b2) * float32(1/3)
 * formed in registers at the load (the sum, at most 765, is exact as an integer and as a float32, so channel order cannot matter; one
 * multiply by the float32 reciprocal, never a division by 3).  That is silent_value_from_color on the widened frame bit for bit, so
 * every output is IDENTICAL to that of the float32-frame entry point given the frame of v values: silent_pyramid[_dev],
 * silent_gray_pass_parts_dev (maps_f16 = 0), silent_gray_pass_h_dev (maps_f16 = 1) and silent_gray_keypoints[_dev] -- without the cast
 * launch, the value launch and the two float32 copies of the batch.  The host-pointer forms stage 3 * H * W * n_frames BYTES of frames.
 * SILENT_E_INVALID as for *_u8; SILENT_E_UNSUPPORTED for a 3-channel plan, a SILENT_PLAN_ACCUM_F64 plan, n_orient other than 3, 4, 8.
 * (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
int silent_pyramid_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, float* pyr);
int silent_pyramid_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, float* pyr,
                            silent_stream stream);
int silent_gray_pass_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                          void* end_out, int maps_f16);
int silent_gray_pass_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                              const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                              void* end_out, int maps_f16, unsigned parts, silent_stream stream);

/* Interleaved 3-channel uint8 frames for 3-CHANNEL plans, read as they are (the *_u8x3 forms above reduce colour to one value for a
 * single-channel plan; these keep the three channels: the RGB pyramid that silent_rgb_line_end / silent_rgb_keypoints read).
 * frames: [n_frames, H, W, 3] bytes, packed, ANY alignment.  Byte c of pixel (y, x) enters the arithmetic as (float)byte -- an unsigned
 * load and an exact conversion in a register -- so pyr is IDENTICAL, bit for bit, to silent_pyramid[_dev] given (float)frames[i], on
 * every route (the single-read walk kernel, union and per-level plans, the unit + region kernels, under every SILENT_TUNE_PYRAMID
 * value): no cast launch and no float32 copy of the batch.  No byte outside the n_frames * H * W * 3 bytes of the batch is ever read:
 * a batch whose address is not 4-byte aligned, or whose W is not a multiple of 4, is read one byte per load, never by aligned-down
 * dword loads.  The host-pointer form stages n_frames * H * W * 3 BYTES of frames; the _dev form is stream-ordered and asynchronous.
 * SILENT_E_INVALID: a NULL plan / frames / pyr, a plan of another context, n_frames < 1 (in this order); SILENT_E_UNSUPPORTED: a
 * single-channel plan (such a plan takes colour bytes through silent_pyramid_u8x3).  (ABI additions only: SILENT_ABI_VERSION is
 * unchanged.) */
int silent_pyramid_rgb8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, float* pyr);
int silent_pyramid_rgb8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, float* pyr,
                            silent_stream stream);

/* Strided uint8 frames, read in place. A decoder hands over NV12 surfaces with a row pitch, a camera or compositor BGRA / BGRX, YUYV
 * carries luma on every second byte, a region of interest is a view with its parent's row step, hipMallocPitch pads rows: none of
 * these is the packed layout of the *_u8 / *_u8x3 entry points, and packing them first is a launch that reads and writes the whole
 * batch plus a second copy of it in device memory.  A view is a base pointer and three BYTE strides (byte, not pixel: a pitched BGR
 * row need not be a multiple of 3); pixel (frame f, row y, column x) is the `channels` bytes at
 *     data + f * frame_stride + y * row_stride + x * pixel_stride        (64-bit arithmetic)
 * with H, W the plan's frame size.  A call reads only bytes of [data, data + span),
 *     span = (n_frames - 1) * frame_stride + (H - 1) * row_stride + (W - 1) * pixel_stride + channels,
 * and inside it only the `channels` bytes of each addressed pixel: never the fourth byte of a BGRA pixel, never a row's padding. */
typedef struct silent_frame_view {
    const uint8_t* data;   /* byte 0 of pixel (0, 0) of frame 0; NO alignment requirement */
    int channels;          /* 1: value = the byte.  3: value = (b0 + b1 + b2) * float32(1/3) of the bytes at +0, +1, +2 */
    int64_t pixel_stride;  /* bytes; >= channels */
    int64_t row_stride;    /* bytes; >= (W - 1) * pixel_stride + channels */
    int64_t frame_stride;  /* bytes; >= (H - 1) * row_stride + (W - 1) * pixel_stride + channels; not read when n_frames == 1 */
} silent_frame_view;

/* The twins of the *_u8 entry points on a view: the same argument lists with `const silent_frame_view* frames` in place of the packed
 * bytes (maps_f16, parts and stream included), the same status codes, and every output IDENTICAL, bit for bit, to that of the *_u8
 * (channels = 1) / *_u8x3 (channels = 3) entry point on the compacted copy of the same pixels.  Single-channel plans without
 * SILENT_PLAN_ACCUM_F64, as there.  In addition SILENT_E_INVALID for a NULL view, NULL data, channels other than 1 or 3, or a stride
 * below its bound (zero and negative strides among them: views are never flipped or broadcast), or a span above 2^63 - 1 bytes.  A view that IS packed --
 * pixel_stride == channels, row_stride == W * pixel_stride, frame_stride == H * row_stride (or n_frames == 1) -- runs the kernels of
 * the packed entry point; any other view runs their strided instantiations (frame and row terms of the address in scalar registers,
 * the column term per lane).  _dev forms: data is a device pointer (the struct itself is host memory, read before the call returns).
 * Host-pointer forms: data is host memory, exactly `span` bytes of it are staged; they refuse what their _dev form refuses before
 * anything is staged.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
int silent_pyramid_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames, float* pyr);
int silent_pyramid_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                            float* pyr, silent_stream stream);
int silent_gray_pass_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                          void* end_out, int maps_f16);
int silent_gray_pass_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                              const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                              void* end_out, int maps_f16, unsigned parts, silent_stream stream);

/* Strided uint8 COLOUR views for 3-CHANNEL plans, read in place: the twins of silent_pyramid_rgb8[_dev] on a silent_frame_view -- the
 * first three bytes of BGRA / BGRX / RGBA pixels, a pitched BGR surface, a region of larger frames, every second pixel.  The struct is
 * taken as it is; channels must be 3.  Pixel (f, y, x) is the three bytes at data + f * frame_stride + y * row_stride + x * pixel_stride
 * (+0, +1, +2; 64-bit arithmetic), and they enter as the three channels of the plan, each as (float)byte -- an unsigned load and an
 * exact conversion; they are NOT reduced to a value (that is channels = 3 of silent_pyramid_view, for single-channel plans).  Stride
 * bounds and span are those of the struct above.  pyr is IDENTICAL, bit for bit, to silent_pyramid_rgb8[_dev] on the compacted copy
 * of the same pixels -- so to silent_pyramid[_dev] on the widened frames -- on every route: the walk kernel, union plans with their
 * border blocks inside the walk launch or behind it, per-level plans, the unit + region kernels, every SILENT_TUNE_PYRAMID value.
 * Reads: only bytes of [data, data + span).  UNLIKE the single-channel view entry points, a byte inside the span that is not a pixel
 * byte (the X of BGRX, row padding) MAY be loaded and dropped; it never influences a result.  The byte behind the last pixel of the
 * batch lies outside the span and is never loaded.  (As built, every load is a single channel byte of a pixel of the view, at any
 * stride and alignment; the wider licence is for a loader that fetches a 4-byte pixel as one dword.)
 * A packed view -- pixel_stride == 3, row_stride == 3 W, frame_stride == H * row_stride (or n_frames == 1) -- runs the packed uint8
 * kernels.  Refusals, in this order: a NULL ctx; SILENT_E_INVALID for a NULL plan / view / data, channels != 3, a stride below its
 * bound, a span above 2^63 - 1 bytes; then those of silent_pyramid_rgb8 (a NULL pyr, a plan of another context, n_frames < 1:
 * SILENT_E_INVALID; a single-channel plan: SILENT_E_UNSUPPORTED -- such a plan takes a view through silent_pyramid_view).  The host
 * form stages exactly `span` bytes and refuses everything its _dev form refuses before anything is staged; the _dev form is
 * stream-ordered and asynchronous.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
int silent_pyramid_rgb8_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames, float* pyr);
int silent_pyramid_rgb8_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                 float* pyr, silent_stream stream);

/* NV12 decoder surfaces for 3-CHANNEL plans, read in place: a full-resolution luma plane `y` and a half-resolution plane `uv` of
 * interleaved (U, V) byte pairs, both pitched, as a hardware video decoder emits them.  Strides are in bytes, 64-bit.  For pixel (y, x)
 * of frame f, with H x W the frame extents of the plan, the value of channel k in {0, 1, 2} is
 *     Yv = (float)y [f * y_frame_stride  + y * y_row_stride + x] - oy
 *     Uv = (float)uv[f * uv_frame_stride + (y >> 1) * uv_row_stride + 2 * (x >> 1)    ] - 128
 *     Vv = (float)uv[f * uv_frame_stride + (y >> 1) * uv_row_stride + 2 * (x >> 1) + 1] - 128
 *     c_k = min(max((Yv * m[3 k] + Uv * m[3 k + 1]) + Vv * m[3 k + 2], 0), 255)
 * with every product and every sum a SEPARATELY ROUNDED float32 operation (no fused multiply-add), chroma NEAREST (a 2 x 2 luma block
 * shares one pair) and NO rounding to an integer: the float32 value enters the pyramid.  Row k of m is channel k, so channel order
 * (BGR / RGB), BT.601 / BT.709 and limited / full range are the caller's choice of m and oy.  The conversion happens in registers at
 * the kernels' loads: no conversion launch, no copy of the batch.  pyr is IDENTICAL, bit for bit, to silent_pyramid[_dev] on the frames
 * silent_nv12_to_rgb[_dev] writes for the same struct, on every route: the walk kernel, union plans with their border blocks, per-level
 * plans, the unit + region kernels, every SILENT_TUNE_PYRAMID value.  Reads: only bytes of [y, y + y_span) and [uv, uv + uv_span),
 * y_span = (n - 1) y_frame_stride + (H - 1) y_row_stride + W, uv_span = (n - 1) uv_frame_stride + (H / 2 - 1) uv_row_stride + W; every
 * load is a luma byte or the pair of a pixel, at any alignment.  A frame stride is not read when n_frames == 1.
 * Refusals, in this order: a NULL ctx; SILENT_E_INVALID for a NULL plan / struct / y / uv, an odd H or W of the plan (4:2:0), a row
 * stride below W, a frame stride below its plane's extent (n_frames > 1), a span above 2^63 - 1 bytes, a non-finite m or oy; then a
 * NULL pyr / rgb, a plan of another context, n_frames < 1 (SILENT_E_INVALID) and a single-channel plan (SILENT_E_UNSUPPORTED: such a
 * plan reads the luma plane through silent_pyramid_view).  The host forms stage exactly the two spans and refuse everything their _dev
 * forms refuse before anything is staged; the _dev forms are stream-ordered and asynchronous; the struct is dead at return.
 * silent_nv12_to_rgb[_dev] writes the converted frames themselves, [n_frames, H, W, 3] float32 -- the frames the pyramid kernels see --
 * with the same device function, one thread per pixel; H and W are arguments (both even, >= 2), refusals as above under its own name.
 * (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
typedef struct silent_nv12_frames {
    const uint8_t* y;
    const uint8_t* uv;
    int64_t y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride;
    float m[9];
    float oy;
} silent_nv12_frames;
int silent_pyramid_nv12(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_nv12_frames* frames, int n_frames, float* pyr);
int silent_pyramid_nv12_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_nv12_frames* frames, int n_frames, float* pyr,
                            silent_stream stream);
int silent_nv12_to_rgb(silent_ctx* ctx, const silent_nv12_frames* frames, int n_frames, int H, int W, float* rgb);
int silent_nv12_to_rgb_dev(silent_ctx* ctx, const silent_nv12_frames* frames, int n_frames, int H, int W, float* rgb, silent_stream stream);

/* P010 / P012 / P016 decoder surfaces for 3-CHANNEL plans, read in place: what a hardware decoder emits for 10- and 12-bit HEVC / AV1 /
 * VP9 -- the NV12 layout with little-endian uint16 elements (native byte order) whose code value of depth d in {10, 12, 16} sits in the
 * HIGH d bits; shift = 16 - d.  Luma `y` is [n, H, W] elements, chroma `uv` [n, H / 2, W / 2, 2] interleaved (U, V) element pairs, both
 * pitched; strides are in BYTES, 64-bit, and even.  For pixel (y, x) of frame f, with Y, U, V the pixel's luma element and the first and
 * second element of its chroma pair (row y >> 1, pair x >> 1), the value of channel k in {0, 1, 2} is
 *     Yv = (float)(Y >> shift) - oy       Uv = (float)(U >> shift) - oc       Vv = (float)(V >> shift) - oc
 *     c_k = min(max((Yv * m[3 k] + Uv * m[3 k + 1]) + Vv * m[3 k + 2], 0), 255)
 * with the elements loaded UNSIGNED (a code >= 0x8000 does not go negative), the low `shift` bits never influencing a result (decoders
 * do not promise zeros there), every difference, product and sum a SEPARATELY ROUNDED float32 operation (no fused multiply-add), chroma
 * NEAREST and NO rounding to an integer: the result is on the 0 .. 255 scale, so a 10-bit code lands on a quarter step of it and keeps
 * its two extra bits.  m, oy, oc and shift are arguments: one set of kernels serves the three depths, every matrix, range and channel
 * order.  With m the NV12 matrix times 2^-(d - 8), oy = 16 * 2^(d - 8) and oc = 128 * 2^(d - 8) (limited range), a surface of elements
 * (byte << 8) | anything-in-the-low-bits gives the pyramid silent_pyramid_nv12 gives for the bytes, bit for bit.
 * The conversion happens in registers at the kernels' loads.  pyr is IDENTICAL, bit for bit, to silent_pyramid[_dev] on the frames
 * silent_p010_to_rgb[_dev] writes for the same struct, on every route: the walk kernel, union plans with their border blocks, per-level
 * plans, the unit + region kernels, every SILENT_TUNE_PYRAMID value.  Reads: only bytes of [y, y + y_span) and [uv, uv + uv_span),
 * y_span = (n - 1) y_frame_stride + (H - 1) y_row_stride + 2 W, uv_span = (n - 1) uv_frame_stride + (H / 2 - 1) uv_row_stride + 2 W;
 * every load is a luma element (2 bytes) or the pair of a pixel (4 bytes at a 2-byte aligned address), nothing outside an addressed
 * element.  A frame stride is not read when n_frames == 1.
 * Refusals, in this order: a NULL ctx; SILENT_E_INVALID for a NULL plan / struct / y / uv, an odd H or W of the plan (4:2:0), a row
 * stride below 2 W, a frame stride below its plane's extent (n_frames > 1), a span above 2^63 - 1 bytes, a non-finite m, oy or oc, an
 * odd y or uv address, an odd stride, a shift outside 0 .. 6; then a NULL pyr / rgb, a plan of another context, n_frames < 1
 * (SILENT_E_INVALID) and a single-channel plan (SILENT_E_UNSUPPORTED: such a plan reads the luma plane through silent_pyramid_view16).
 * The host forms stage exactly the two spans and refuse everything their _dev forms refuse before anything is staged; the _dev forms
 * are stream-ordered and asynchronous; the struct is dead at return.  silent_p010_to_rgb[_dev] writes the converted frames themselves,
 * [n_frames, H, W, 3] float32, with the same device functions, one thread per pixel; H and W are arguments (both even, >= 2), refusals
 * as above under its own name.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
typedef struct silent_p010_frames {
    const uint16_t* y;
    const uint16_t* uv;
    int64_t y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride;
    float m[9];
    float oy;
    float oc;
    int shift;
} silent_p010_frames;
int silent_pyramid_p010(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_p010_frames* frames, int n_frames, float* pyr);
int silent_pyramid_p010_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_p010_frames* frames, int n_frames, float* pyr,
                            silent_stream stream);
int silent_p010_to_rgb(silent_ctx* ctx, const silent_p010_frames* frames, int n_frames, int H, int W, float* rgb);
int silent_p010_to_rgb_dev(silent_ctx* ctx, const silent_p010_frames* frames, int n_frames, int H, int W, float* rgb, silent_stream stream);

/* Planar and packed 8-bit YUV for 3-CHANNEL plans, read in place: what software decoders (I420 / YV12), GPU JPEG decoders (planar
 * 4:2:2 / 4:4:4), UVC webcams (YUYV / UYVY) and Android / capture cards (NV21) emit.  These formats differ from NV12 in ADDRESSING
 * only, so one struct describes them all: three plane pointers (they may overlap: a packed format is three views of one buffer; they
 * are only read), a pixel stride per plane class, a chroma subsampling shift per axis (0 or 1).  Strides are in BYTES, 64-bit.  With
 * sx = chroma_shift_x, sy = chroma_shift_y, pixel (y, x) of frame f reads the three bytes
 *     Y = y[f y_frame_stride + y y_row_stride + x y_pixel_stride]
 *     U = u[f c_frame_stride + (y >> sy) c_row_stride + (x >> sx) c_pixel_stride]        V = v[the same offset]
 * and the value of channel k in {0, 1, 2} is
 *     Yv = (float)Y - oy       Uv = (float)U - 128       Vv = (float)V - 128
 *     c_k = min(max((Yv * m[3 k] + Uv * m[3 k + 1]) + Vv * m[3 k + 2], 0), 255)
 * -- NV12's conversion to the letter: every product and sum a SEPARATELY ROUNDED float32 operation (no fused multiply-add), chroma
 * NEAREST, NO rounding to an integer.
 *     I420 / YV12: three planes, shifts 1 / 1 (YV12: u and v swapped)      I422, I444, 4:4:0: shifts 1 / 0, 0 / 0, 0 / 1
 *     NV12: u = uv, v = uv + 1, c_pixel_stride = 2      NV21: v = vu, u = vu + 1      NV16 / NV24: the same with shifts 1 / 0, 0 / 0
 *     YUYV: y = base, y_pixel_stride = 2, u = base + 1, v = base + 3, c_pixel_stride = 4, shifts 1 / 0 (UYVY: y = base + 1, u = base, v = base + 2)
 *     VUYA / AYUV: all pixel strides 4, shifts 0 / 0
 * The conversion happens in registers at the kernels' loads.  pyr is IDENTICAL, bit for bit, to silent_pyramid[_dev] on the frames
 * silent_yuv_to_rgb[_dev] writes for the same struct, on every route: the walk kernel, union plans with their border blocks (inside
 * and behind the walk's launch), per-level plans, the unit + region kernels, every SILENT_TUNE_PYRAMID value.  A struct that IS NV12
 * (y_pixel_stride == 1, c_pixel_stride == 2, v == u + 1, shifts 1 / 1) runs the kernels of silent_pyramid_nv12 and gives its bits.
 * Reads: every load is ONE BYTE that is some pixel's Y, U or V -- no pair loads, no dword loads; nothing between pixels is ever read
 * and nothing outside the three spans, the span of a plane being (n - 1) frame_stride + (rows - 1) row_stride + (cols - 1)
 * pixel_stride + 1 with rows x cols = H x W for y and (H >> sy) x (W >> sx) for u and v.  (The NV12 kernels read the (U, V) bytes of a
 * pixel as one pair: the same bytes.)  A frame stride is not read when n_frames == 1.
 * Refusals, in this order: a NULL ctx; SILENT_E_INVALID for a NULL plan / struct / y / u / v, a shift other than 0 or 1, an odd H with
 * chroma_shift_y = 1 or an odd W with chroma_shift_x = 1 (or H, W < 1), a pixel stride < 1, a row stride below its plane's row extent
 * (cols - 1) pixel_stride + 1, a frame stride below its plane's extent (n_frames > 1), a span above 2^63 - 1 bytes, a non-finite m or
 * oy; then a NULL pyr / rgb, a plan of another context, n_frames < 1 (SILENT_E_INVALID) and a single-channel plan
 * (SILENT_E_UNSUPPORTED: such a plan reads the luma plane through silent_pyramid_view).
 * The host forms refuse everything their _dev forms refuse before anything is staged, and stage the UNION of the three spans: the
 * intervals sorted, those that overlap or touch merged, each merged interval copied once, the pointers rebased -- a YUYV buffer
 * crosses the bus once, not three times.  The _dev forms are stream-ordered and asynchronous; the struct is dead at return.
 * silent_yuv_to_rgb[_dev] writes the converted frames themselves, [n_frames, H, W, 3] float32, with the same device functions, one
 * thread per pixel; H and W are arguments, refusals as above under its own name.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
typedef struct silent_yuv_frames {
    const uint8_t* y;
    const uint8_t* u;
    const uint8_t* v;
    int64_t y_pixel_stride, y_row_stride, y_frame_stride;
    int64_t c_pixel_stride, c_row_stride, c_frame_stride;
    int32_t chroma_shift_x, chroma_shift_y;
    float m[9];
    float oy;
} silent_yuv_frames;
int silent_pyramid_yuv(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv_frames* frames, int n_frames, float* pyr);
int silent_pyramid_yuv_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv_frames* frames, int n_frames, float* pyr,
                           silent_stream stream);
int silent_yuv_to_rgb(silent_ctx* ctx, const silent_yuv_frames* frames, int n_frames, int H, int W, float* rgb);
int silent_yuv_to_rgb_dev(silent_ctx* ctx, const silent_yuv_frames* frames, int n_frames, int H, int W, float* rgb, silent_stream stream);

/* Planar, semi-planar and packed 16-BIT YUV for 3-CHANNEL plans, read in place: what software decoders (FFmpeg, dav1d, libaom, libvpx)
 * emit for HEVC Main10 / AV1 / VP9 profile 2 (yuv420p10le / I010 and its 4:2:2, 4:4:4 and 12-bit siblings: the code in the LOW bits),
 * the semi-planar 4:2:2 / 4:4:4 surfaces P210 / P216 / P410 / P416 and the packed Y210 / Y216 / Y416 (the code in the HIGH bits).
 * silent_yuv_frames' addressing with silent_p010_frames' arithmetic: three plane pointers of little-endian uint16 elements (native byte
 * order; they may overlap: a packed format is three views of one buffer; they are only read), a pixel stride per plane class, a chroma
 * subsampling shift per axis (0 or 1).  Strides are in BYTES, 64-bit, and EVEN.  With sx = chroma_shift_x, sy = chroma_shift_y, pixel
 * (y, x) of frame f reads the three elements at the byte offsets
 *     Y: f y_frame_stride + y y_row_stride + x y_pixel_stride                                       from y
 *     U: f c_frame_stride + (y >> sy) c_row_stride + (x >> sx) c_pixel_stride   from u,       V: the same offset from v
 * and the value of channel k in {0, 1, 2} is
 *     code(e) = (e >> shift) & ((1 << depth) - 1)                     e loaded UNSIGNED (a code >= 0x8000 does not go negative)
 *     Yv = (float)code(Y) - oy       Uv = (float)code(U) - oc       Vv = (float)code(V) - oc
 *     c_k = min(max((Yv * m[3 k] + Uv * m[3 k + 1]) + Vv * m[3 k + 2], 0), 255)
 * -- P010's conversion to the letter: every difference, product and sum a SEPARATELY ROUNDED float32 operation (no fused multiply-add),
 * chroma NEAREST, NO rounding to an integer, the result on the 0 .. 255 scale.  Bits of an element outside [shift, shift + depth) never
 * influence a result.  The code in the high bits: shift = 16 - depth; in the low bits: shift = 0.  8 <= depth <= 16, shift >= 0,
 * shift + depth <= 16.
 *     I010 / I210 / I410 (yuv420p10le / yuv422p10le / yuv444p10le; I012 ...: depth 12): three planes, y_pixel_stride = c_pixel_stride = 2,
 *                                                                    shifts 1 / 1, 1 / 0, 0 / 0, shift = 0
 *     P010 / P210 / P410 (P016 / P216 / P416: depth 16): u = uv, v = uv + 1 element, c_pixel_stride = 4, shifts 1 / 1, 1 / 0, 0 / 0,
 *                                                                    shift = 16 - depth; a VU order (NV21-like): v = vu, u = vu + 1
 *     Y210 / Y216 (Y0 U Y1 V): y = base, y_pixel_stride = 4, u = base + 1, v = base + 3 elements, c_pixel_stride = 8, shifts 1 / 0,
 *                                                                    shift = 16 - depth
 *     Y416 (U Y V A): u = base, y = base + 1, v = base + 2 elements, all pixel strides 8, shifts 0 / 0, depth 16
 *     4:4:0: shifts 0 / 1
 * The conversion happens in registers at the kernels' loads.  pyr is IDENTICAL, bit for bit, to silent_pyramid[_dev] on the frames
 * silent_yuv16_to_rgb[_dev] writes for the same struct, on every route: the walk kernel, union plans with their border blocks (inside
 * and behind the walk's launch), per-level plans, the unit + region kernels, every SILENT_TUNE_PYRAMID value.  A struct that IS P010
 * (y_pixel_stride == 2, c_pixel_stride == 4, v == u + 1 element, shifts 1 / 1, shift == 16 - depth) runs the kernels of
 * silent_pyramid_p010 and gives its bits.
 * Reads: every load is ONE 2-byte element at a 2-byte aligned address that is some pixel's Y, U or V: no pair loads, no dword loads,
 * nothing between pixels, nothing outside the three spans, the span of a plane being (n - 1) frame_stride + (rows - 1) row_stride +
 * (cols - 1) pixel_stride + 2 bytes with rows x cols = H x W for y and (H >> sy) x (W >> sx) for u and v.  (The P010 kernels read the
 * (U, V) elements of a pixel as one pair: the same bytes.)  A frame stride is not read when n_frames == 1.
 * Refusals, in this order: a NULL ctx; SILENT_E_INVALID for a NULL plan / struct / y / u / v, a chroma shift other than 0 or 1, an odd H
 * with chroma_shift_y = 1 or an odd W with chroma_shift_x = 1 (or H, W < 1), a pixel stride < 2, a row stride below its plane's row
 * extent (cols - 1) pixel_stride + 2, a frame stride below its plane's extent (n_frames > 1), a span above 2^63 - 1 bytes, a non-finite
 * m, oy or oc, an odd y, u or v address, an odd stride, a depth outside 8 .. 16 or a shift outside 0 .. 16 - depth; then a NULL pyr /
 * rgb, a plan of another context, n_frames < 1 (SILENT_E_INVALID) and a single-channel plan (SILENT_E_UNSUPPORTED: such a plan reads
 * the luma plane through silent_pyramid_view16).
 * The host forms refuse everything their _dev forms refuse before anything is staged, and stage the UNION of the three spans: the
 * intervals sorted, those that overlap or touch merged, each merged interval copied once, the pointers rebased -- a Y210 buffer
 * crosses the bus once, not three times.  The _dev forms are stream-ordered and asynchronous; the struct is dead at return.
 * silent_yuv16_to_rgb[_dev] writes the converted frames themselves, [n_frames, H, W, 3] float32, with the same device functions, one
 * thread per pixel; H and W are arguments, refusals as above under its own name.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
typedef struct silent_yuv16_frames {
    const uint16_t* y;
    const uint16_t* u;
    const uint16_t* v;
    int64_t y_pixel_stride, y_row_stride, y_frame_stride;
    int64_t c_pixel_stride, c_row_stride, c_frame_stride;
    int32_t chroma_shift_x, chroma_shift_y;
    float m[9];
    float oy;
    float oc;
    int32_t shift;
    int32_t depth;
} silent_yuv16_frames;
int silent_pyramid_yuv16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv16_frames* frames, int n_frames, float* pyr);
int silent_pyramid_yuv16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv16_frames* frames, int n_frames, float* pyr,
                             silent_stream stream);
int silent_yuv16_to_rgb(silent_ctx* ctx, const silent_yuv16_frames* frames, int n_frames, int H, int W, float* rgb);
int silent_yuv16_to_rgb_dev(silent_ctx* ctx, const silent_yuv16_frames* frames, int n_frames, int H, int W, float* rgb, silent_stream stream);

/* Raw 8-bit Bayer mosaics, read in place: what machine-vision and robotics cameras on GigE Vision, USB3 Vision or MIPI deliver
 * (BayerRG8 / BayerGR8 / BayerGB8 / BayerBG8) -- ONE BYTE per pixel, the colours in a 2 x 2 pattern, a third of packed BGR.  One plane:
 * m(f, y, x) is the byte at data + f * frame_stride + y * row_stride + x * pixel_stride, strides in bytes and positive, frame and row
 * terms 64-bit -- a pitched buffer, a window of a larger sensor image and every-second-byte layouts are all just strides.  H, W >= 2,
 * odd extents allowed.
 * pattern names the top-left 2 x 2 cell of THE VIEW THAT IS PASSED (a window that starts on an odd row or column of a sensor has another
 * name than the sensor):            red at (y & 1, x & 1)   blue at
 *     0  rggb (BayerRG8)                 (0, 0)             (1, 1)
 *     1  grbg (BayerGR8)                 (0, 1)             (1, 0)
 *     2  gbrg (BayerGB8)                 (1, 0)             (0, 1)
 *     3  bggr (BayerBG8)                 (1, 1)             (0, 0)
 * order: 0 = channels (b, g, r), 1 = (r, g, b).
 * The conversion is BILINEAR demosaicing in registers at the kernels' loads.  Indices outside the frame are reflected without repeating
 * the edge (-1 -> 1, H -> H - 2, the same along x): reflection keeps the parity of an index, so a reflected neighbour has the colour
 * its position calls for.  Every pixel gets three float32 channels:
 *     at a red or blue site:  its own colour (float)m(y, x);  green (m(y-1,x) + m(y+1,x) + m(y,x-1) + m(y,x+1)) * 0.25;  the opposite
 *                             colour (the four diagonal neighbours) * 0.25
 *     at a green site:        green (float)m(y, x);  the colour whose samples lie in the same row (m(y,x-1) + m(y,x+1)) * 0.5;  the other
 *                             colour (m(y-1,x) + m(y+1,x)) * 0.5
 * Each sum is an integer (at most 1020), converted once to float32 and multiplied once by 0.25 or 0.5 -- all exact: the value is a
 * multiple of 1/4 in [0, 255], is NOT rounded to an integer and has the same bits in any evaluation order.
 * This is NOT OpenCV's COLOR_Bayer*2BGR, which rounds to uint8 and treats the border differently; and OpenCV's pattern names are
 * shifted against the sensor's (its "BayerBG" is a sensor's RGGB): go by the table above, not by OpenCV's constant.
 * pyr is IDENTICAL, bit for bit, to silent_pyramid[_dev] on the frames silent_bayer_to_rgb[_dev] writes for the same struct, on every
 * route: the walk kernel, union plans with their border blocks (inside and behind the walk's launch), per-level plans, the unit +
 * region kernels, every SILENT_TUNE_PYRAMID value.  A crop of a plan that starts on an odd row or column reads the FRAME's parity.
 * Reads: every load is ONE BYTE that is some pixel of the view -- nothing between pixels (pixel_stride > 1), nothing behind a row's W
 * pixels, nothing outside [data, data + span), span = (n - 1) frame_stride + (H - 1) row_stride + (W - 1) pixel_stride + 1.  The frame
 * stride is not read when n_frames == 1.
 * Refusals, before any launch or staging: a NULL ctx; SILENT_E_INVALID for a NULL plan / struct / data, a pattern outside 0 .. 3, an
 * order outside 0 .. 1, H or W below 2, a pixel stride < 1, a row stride below (W - 1) pixel_stride + 1, a frame stride below the
 * frame's extent (n_frames > 1), a span above 2^63 - 1 bytes; then a NULL pyr / rgb, a plan of another context, n_frames < 1
 * (SILENT_E_INVALID), a single-channel plan or a SILENT_PLAN_ACCUM_F64 plan (SILENT_E_UNSUPPORTED).
 * The host forms refuse everything their _dev forms refuse before anything is staged, and stage the view's span, not a byte more.  The
 * _dev forms are stream-ordered and asynchronous; the struct is dead at return.
 * silent_bayer_to_rgb[_dev] writes the converted frames themselves, [n_frames, H, W, 3] float32, with the same device function, one
 * thread per pixel; H and W are arguments, refusals as above under its own name.  8-bit mosaics only: 10 / 12 / 16-bit mosaics, a
 * gray value from a mosaic and higher-order demosaicing are not provided.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
typedef struct silent_bayer_frames {
    const uint8_t* data;
    int64_t pixel_stride, row_stride, frame_stride;
    int32_t pattern;
    int32_t order;
} silent_bayer_frames;
int silent_pyramid_bayer(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_bayer_frames* frames, int n_frames, float* pyr);
int silent_pyramid_bayer_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_bayer_frames* frames, int n_frames, float* pyr,
                             silent_stream stream);
int silent_bayer_to_rgb(silent_ctx* ctx, const silent_bayer_frames* frames, int n_frames, int H, int W, float* rgb);
int silent_bayer_to_rgb_dev(silent_ctx* ctx, const silent_bayer_frames* frames, int n_frames, int H, int W, float* rgb, silent_stream stream);

/* uint16 frames, read as they are: 10 / 12 / 16-bit machine-vision and scientific cameras (Mono10 / Mono12 / Mono16), thermal and
 * depth sensors (Y16, Z16), 16-bit TIFF / PNG, and the luma of the P010 / P016 surfaces a hardware decoder hands over for 10-bit
 * HEVC / AV1.  The twins of the *_u8 entry points -- same argument lists, maps_f16 / parts / stream arguments, status codes and order
 * of refusals -- for frames: [n_frames, H, W] unsigned 16-bit integers in native byte order, 2-BYTE ALIGNED (an odd address is
 * SILENT_E_INVALID).  The frame-reading kernels load the element UNSIGNED and convert it in a register -- uint16 -> float32 is exact,
 * 65535 < 2^24 -- so every output is IDENTICAL, bit for bit, to that of the float32-frame entry point given (float)frames[i]:
 * silent_pyramid[_dev], silent_gray_pass_parts_dev (maps_f16 = 0), silent_gray_pass_h_dev (maps_f16 = 1) and
 * silent_gray_keypoints[_dev].  The host-pointer forms stage 2 * H * W * n_frames BYTES of frames.
 * No scaling and no shift.  P010 keeps its 10 bits in the HIGH bits of each element (v << 6): the pass is homogeneous of degree one
 * up to clip_hi, and a factor of 64 is exact in binary floating point, so a P010 caller passes clip_hi * 64 and reads maps that are
 * exactly 64 times those of the 10-bit values.
 * float16 maps (maps_f16 = 1) keep their rule -- the float32 result rounded to nearest even, overflow to +-inf: with full-range
 * 16-bit data and clip_hi above 65504 a stored map element can be +inf, exactly where silent_gray_pass_h_dev stores it for the
 * widened frame.
 * Not built: signed int16, interleaved 16-bit colour, 3-channel plans, SILENT_PLAN_ACCUM_F64 plans (both SILENT_E_UNSUPPORTED),
 * byte-swapped data.  (ABI additions only: SILENT_ABI_VERSION is unchanged.) */
int silent_pyramid_u16(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames, float* pyr);
int silent_pyramid_u16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames, float* pyr,
                           silent_stream stream);
int silent_gray_pass_u16(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                         const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                         void* end_out, int maps_f16);
int silent_gray_pass_u16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                             const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                             void* end_out, int maps_f16, unsigned parts, silent_stream stream);

/* Strided uint16 frames, read in place: the valid part of a pitched P010 / P016 surface, one channel of 16-bit RGBA, a window of
 * larger frames.  As silent_frame_view with one uint16 element per pixel: pixel (frame f, row y, column x) is the 2 bytes at
 *     data + f * frame_stride + y * row_stride + x * pixel_stride        (BYTE strides, 64-bit arithmetic)
 * and a call reads only those 2 bytes of each addressed pixel, all inside [data, data + span),
 *     span = (n_frames - 1) * frame_stride + (H - 1) * row_stride + (W - 1) * pixel_stride + 2.
 * The twins of the *_view entry points: every output IDENTICAL, bit for bit, to that of the *_u16 entry point on the compacted copy
 * of the same pixels; status codes and order of refusals as *_view with 2 for `channels`, and in addition SILENT_E_INVALID for an
 * odd data address or an odd stride.  A view that IS packed -- pixel_stride == 2, row_stride == 2 * W, frame_stride == H * row_stride
 * (or n_frames == 1) -- runs the kernels of the *_u16 entry point.  Host-pointer forms stage exactly `span` bytes. */
typedef struct silent_frame_view16 {
    const uint16_t* data;  /* pixel (0, 0) of frame 0; 2-byte aligned */
    int64_t pixel_stride;  /* bytes; even, >= 2 */
    int64_t row_stride;    /* bytes; even, >= (W - 1) * pixel_stride + 2 */
    int64_t frame_stride;  /* bytes; even, >= (H - 1) * row_stride + (W - 1) * pixel_stride + 2; not read when n_frames == 1 */
} silent_frame_view16;
int silent_pyramid_view16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames, float* pyr);
int silent_pyramid_view16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                              float* pyr, silent_stream stream);
int silent_gray_pass_view16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                            const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                            void* end_out, int maps_f16);
int silent_gray_pass_view16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out,
                                void* end_out, int maps_f16, unsigned parts, silent_stream stream);

/* 1 when silent_gray_pass runs this plan through the single-read stream kernel (one unit-zoom level and every
 * other level resampling the same crop with a step > 1.25: classic whole-frame pyramids), 0 when it falls
 * back to region + unit-fused + filter kernels (e.g. the reference's centred-crop layout).  The same for
 * SILENT_PLAN_ACCUM_F64 plans (their own float64 instantiations of the same kernels). */
int silent_pyramid_plan_is_streamable(const silent_pyramid_plan* plan);

/* 3-channel plans: the number of WALK PLANS silent_pyramid runs this pyramid with in ONE launch of the strip-walk kernel (frame rows
 * DMA'd once per crop into an LDS ring): 1 for a classic whole-frame pyramid (unit level + every other level on the same crop), one
 * per level for crop layouts such as the reference's (image_to_zoom_tensor, util/zoom/from_image.py:45-64: nested centre crops); 0
 * when the plan falls back to the unit + region kernels (more than 8 levels of a crop layout; more than 21 outputs per wave tile:
 * zoom steps below 1.6; frame width not a multiple of 4).  pixels_per_wave (may be NULL): 36 or 32. */
int silent_pyramid_plan_walk_plans(const silent_pyramid_plan* plan, int* pixels_per_wave);

/* Optional HIP-event timing of the DOMINANT kernel of the last silent_gray_pass_dev call (the fused
 * unit-level kernel): silent_set_profiling(ctx, n) with n >= 1 brackets that kernel with an event pair on every
 * n-th call (n = 0: off), on the stream the kernel runs on -- an event is a packet in the queue, so bracketing every
 * call costs a few per cent of a millisecond-long pass.  silent_profile_elapsed_ms synchronises and returns the MEAN
 * over the (up to 8 most recent) recorded pairs since the last silent_set_profiling, and the number of
 * level-0-class pixels the kernel processed per launch. */
int silent_set_profiling(silent_ctx* ctx, int enable);
int silent_profile_elapsed_ms(silent_ctx* ctx, float* ms, int64_t* pixels);

/* Kernel-selection knobs for tests and A/B timing (no reference counterpart: the reference has one code path).
 * Every context starts from the environment variables SILENT_GRAY_OPTS / SILENT_RGB_OPTS / SILENT_PYRAMID_OPTS, read
 * once in silent_create; silent_set_tuning changes a knob of one context afterwards.  Bits -- GRAY: 1 XCD-aware tile
 * order, 16 no single-read stream kernel, 32 XCD order in the stream kernel (2 and 8 selected 32-row tiles until round 5: slower in
 * every A/B, the instantiations are gone and the bits are ignored);
 * RGB: 1 dense weights, 2 no two-group form, 8 no short tiles, 16 the one-pixel-per-lane chain kernel (default: two pixels
 * per lane on packed f32, same bits), 32 no sparse keypoint tail, 64 no symmetric forms (the two-group instantiation of the pair
 * kernel, bit-identical to the one-pixel kernel), 128 16-byte stores of orient / line_end where rows are 16-byte aligned (same bits as the default
 * 12-byte form, same speed), bits 8-15 tile height / 2; PYRAMID: 1 no single-read pyramid
 * (gray stream kernel, RGB strip walk), 2 no RGB strip walk.  All variants give the same results (bit-identical, or within
 * the re-association tolerance for the RGB forms); the defaults are the fastest measured. */
#define SILENT_TUNE_GRAY 0
#define SILENT_TUNE_RGB 1
#define SILENT_TUNE_PYRAMID 2
#define SILENT_TUNE_COUNT 3
int silent_set_tuning(silent_ctx* ctx, int which, unsigned value);
int silent_get_tuning(const silent_ctx* ctx, int which, unsigned* value);

/* ---------------------------------------------------------------------------- a-6 regulator
 * Replaces regulate_tensor, slam_recognition/util/regulator/gaussian_regulator_tensor.py:10-36:
 *   y = x * (rv / pow(min(conv(x, blur), 1), root)); blur is HWIO [kh, kw, C, C].
 * The power is powf over the blur's whole range: a denormal blur is not flushed (the factor overflows to inf once
 * pow(b, root) is below rv / FLT_MAX), b = 0 gives rv / 0 = inf (0 * inf = NaN under SILENT_FLAT_IEEE), and a negative
 * blur follows pow: NaN unless root is an integer (root 1: rv / b; root 0: rv).  Within 8 * 2^-24 of |y| of the float64
 * power rounded per op (tests/test_gpu_regulator_domain.py). */
int silent_regulate(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                    int channels, const float* blur_hwio, int kh, int kw, float regulation_value,
                    float regulation_root, int flat_policy, float* out);
int silent_regulate_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                        int channels, const float* blur_hwio, int kh, int kw, float regulation_value,
                        float regulation_root, int flat_policy, float* out, silent_stream stream);

/* ---------------------------------------------------------------------------- a-7 / a-8 pointwise
 * pad_inwards            slam_recognition/util/selection/isolate_rectangle.py:19-23 (multiply by a 0/1 mask)
 * get_value_from_color   slam_recognition/util/color/get_value.py:6-12 (channel sum * float32(1/C)) */
int silent_pad_inwards(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                       int channels, int pad_top, int pad_bottom, int pad_left, int pad_right, float* out);
int silent_pad_inwards_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                           int n_frames, int channels, int pad_top, int pad_bottom, int pad_left, int pad_right,
                           float* out, silent_stream stream);
int silent_value_from_color(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                            int n_frames, int channels, float* out);
int silent_value_from_color_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                int n_frames, int channels, float* out, silent_stream stream);
/* get_bw_from_color      slam_recognition/util/color/get_bw.py:6-13: 1 where the channel sum (x . ones, summed left to
 * right in float32) is not 0 -- NaN counts as not 0, like tf.not_equal -- else 0; one output channel. */
int silent_bw_from_color(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                         int channels, float* out);
int silent_bw_from_color_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                             int n_frames, int channels, float* out, silent_stream stream);

/* ---------------------------------------------------------------------------- a-9 non-max suppression */
int silent_nms3x3(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                  int channels, int mode, float* out);
int silent_nms3x3_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels, int n_frames,
                      int channels, int mode, float* out, silent_stream stream);

/* ---------------------------------------------------------------------------- a-10 top-percent threshold
 * Replaces top_value_points, slam_recognition/util/selection/top_value_points.py:8-29: per level
 * (= per batch item of the reference) thr = (1-p)*max(value) + p*min(value), out = color * (value >= thr).
 * value: packed 1-channel map (NULL -> computed from color as get_value_from_color does). */
int silent_top_value_points(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                            int n_levels, int n_frames, int channels, double top_percent, float* out);
int silent_top_value_points_dev(silent_ctx* ctx, const float* color, const float* value,
                                const silent_extent* levels, int n_levels, int n_frames, int channels,
                                double top_percent, float* out, silent_stream stream);

/* ---------------------------------------------------------------------------- a-11 keypoint indices
 * Replaces max_value_indices_region, slam_recognition/util/selection/top_value_points.py:32-45:
 * tf.where(value >= resize_nearest(max_pool(value, k=(H,W), strides=(rH,rW), SAME))) with the TF1
 * SAME / NEAREST index rules.  regions[l] = (rH, rW) of level l, any extents >= 1: up to
 * 4 x 4 windows per level (the reference uses 2 x 2) run a one-pass cell-maximum path, more windows the separable
 * prefix / suffix path (any level width: the row pass walks a row in chunks); same results either way.
 * idx: n_frames x cap_per_frame x 4 int64 rows (level, y, x, 0), ROW-MAJOR SORTED within a frame like
 * tf.where; counts[f] = number of rows frame f produced.  If any count exceeds cap_per_frame only the
 * first cap_per_frame rows of that frame are written and the host call returns SILENT_E_CAPACITY.
 * The _dev twin leaves counts on the device and cannot report capacity: check counts yourself. */
int silent_max_value_indices_region(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels,
                                    int n_frames, const silent_extent* regions, int64_t* idx,
                                    size_t cap_per_frame, int64_t* counts);
int silent_max_value_indices_region_dev(silent_ctx* ctx, const float* value, const silent_extent* levels,
                                        int n_levels, int n_frames, const silent_extent* regions, int64_t* idx,
                                        size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* ---------------------------------------------------------------------------- fused selection
 * top_value_points (util/selection/top_value_points.py:8-29) -> 3x3 NMS in product form
 * (_experimental/vision_filter.py:88-89) -> get_value_from_color (util/color/get_value.py:6-12) in one streaming
 * pass after the per-level max / min reduction: bit-identical to silent_top_value_points + silent_nms3x3 +
 * silent_value_from_color, without the two intermediate colour maps in HBM.  value may be NULL (computed from color).
 * Any of top_out [C ch], peaks_out [C ch], peak_value_out [1 ch] may be NULL, not all.  channels: 1, 3, 4 or 8. */
int silent_select_peaks(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                        int n_levels, int n_frames, int channels, double top_percent, float* top_out,
                        float* peaks_out, float* peak_value_out);
int silent_select_peaks_dev(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                            int n_levels, int n_frames, int channels, double top_percent, float* top_out,
                            float* peaks_out, float* peak_value_out, silent_stream stream);

/* SURVEY 8d config 3 in one call: silent_select_peaks followed by silent_max_value_indices_region on its peak value
 * (a-10 -> a-9 -> a-8 -> a-11), with the cell maxima of the keypoint search folded into the selection pass (one pass
 * over the value map less).  Outputs exactly as those two calls: peak_value_out [1 ch] (may be NULL: the map then lives in
 * the context workspace), idx / counts as silent_max_value_indices_region. */
int silent_select_keypoints(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                            int n_levels, int n_frames, int channels, double top_percent,
                            const silent_extent* regions, float* peak_value_out, int64_t* idx, size_t cap_per_frame,
                            int64_t* counts);
int silent_select_keypoints_dev(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                                int n_levels, int n_frames, int channels, double top_percent,
                                const silent_extent* regions, float* peak_value_out, int64_t* idx,
                                size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* ---------------------------------------------------------------------------- centroids
 * Replaces get_centroids, slam_recognition/util/centroids.py:21-46 (with index_tensor.from_shape,
 * util/index_tensor.py:7-20, dimensions reversed: channel 0 = x, channel 1 = y): per cell of region_h x
 * region_w pixels (window = stride, TF SAME geometry) the value-weighted centroid; every pixel gets the L1
 * distance to the centroid of its (nearest-neighbour) cell.  Empty cells give 0/0 = NaN like the reference.
 * value: packed 1-channel maps.  dist_out: same geometry.  total_out: packed cell maps, level l has
 * ceil(h_l / region_h) x ceil(w_l / region_w) cells (the reference's total_pool). */
int silent_centroids(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels, int n_frames,
                     int region_h, int region_w, float* dist_out, float* total_out);
int silent_centroids_dev(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels,
                         int n_frames, int region_h, int region_w, float* dist_out, float* total_out,
                         silent_stream stream);

/* ---------------------------------------------------------------------------- boosting state
 * Replaces get_boosting, slam_recognition/util/energy/boosting.py:10-42 with generate_recovery,
 * util/energy/recovery.py:4-22.  The state ("exhaustion_tensor", a tf.Variable in the reference,
 * recognition_testing.py:56) is a caller-owned float buffer with the geometry of the input, updated IN PLACE:
 *     m      = input ** energy                      (float64 pow rounded to float32)
 *     fired  = (m == maxpool3x3 SAME (m)) ? 1 : 0
 *     energy = clip((energy*255 - fired*255 + recovery) / 255, -exhaustion_max, +excitation_max)
 * Saving / restoring a stream is a copy of that buffer (initial value: 8 everywhere, boosting.py:6-7).  Each frame
 * slot of the batch is its own stream; successive calls advance every stream by one step, so the frames of one
 * stream must come to the same slot, in order.
 * visualize = 0: fired_out and energy_out (may be NULL) have 1 channel (has_fired, new energy).
 * visualize = 1 (for_visualizing, boosting.py:35-40): both have 3 identical channels, fired * input and
 *                energy * 255/(exhaustion_max+excitation_max) + 255*excitation_max/(exhaustion_max+excitation_max). */
#define SILENT_RECOVERY_CONSTANT 1u
#define SILENT_RECOVERY_INPUT 2u

typedef struct silent_boosting_params {
    float exhaustion_max;      /* 1 */
    float excitation_max;      /* 1 */
    unsigned recovery_mode;    /* SILENT_RECOVERY_CONSTANT (reference default) | SILENT_RECOVERY_INPUT */
    float recovery_amount;     /* 10   (recovery.py:4) */
    float recovery_percentage; /* 0.8  (recovery.py:8) */
    int32_t visualize;
} silent_boosting_params;

int silent_boosting_step(silent_ctx* ctx, const float* input, const silent_extent* levels, int n_levels,
                         int n_frames, const silent_boosting_params* params, float* energy, float* fired_out,
                         float* energy_out);
int silent_boosting_step_dev(silent_ctx* ctx, const float* input, const silent_extent* levels, int n_levels,
                             int n_frames, const silent_boosting_params* params, float* energy, float* fired_out,
                             float* energy_out, silent_stream stream);

/* ---------------------------------------------------------------------------- display-graph glue
 * The scalar ops between the kernels of LineEndDisplayer.compile, recognition_testing.py:79-81 and :99
 * (``t / 255.0``, ``clip_by_value(t * (255 / 4.0), 1, 256) - 1``, ``255 - t * 255``, ``t * 255``):
 *     out[i] = clip(in[i] * mul / div + add, lo, hi) + post_add        (float32, one rounding per operation;
 * mul = div = 1, add = post_add = 0, lo = -INFINITY, hi = +INFINITY are the neutral values).  in == out is allowed. */
typedef struct silent_affine_params {
    float mul, div, add, lo, hi, post_add;
} silent_affine_params;

int silent_affine_clip(silent_ctx* ctx, const float* in, size_t n_values, const silent_affine_params* params,
                       float* out);
int silent_affine_clip_dev(silent_ctx* ctx, const float* in, size_t n_values, const silent_affine_params* params,
                           float* out, silent_stream stream);

/* np.asarray(frame, dtype=np.float32) (slam_recognition/recognition_testing.py:141: the camera's uint8 frame becomes the
 * float32 tensor the pyramid takes) and the colour-plane slicing of image_to_zoom_tensor (util/zoom/from_image.py:54-64,
 * one scipy zoom per plane) as ONE strided cast on the device:
 *     out[p * out_stride + out_offset + k] = (float)in[p * in_stride + in_offset + k]      p < n_pixels, k < count
 * (strides / offsets in ELEMENTS).  in_dtype: SILENT_DT_*.  Widening (strides = count = channels), cutting plane c out of
 * an interleaved image (in_stride = C, in_offset = c, count = 1, out_stride = 1) and interleaving planes back are all
 * instances.  in and out must not overlap.  The conversion is the C cast: exact for uint8 / int16 / uint16 and for integers up to
 * 2^24 in magnitude, round-to-nearest-even beyond (int32 / int64 / float64), like numpy's astype(float32).  Buffer sizes: `in`
 * holds at least (n_pixels - 1) * in_stride + in_offset + count elements, `out` (n_pixels - 1) * out_stride + out_offset + count
 * floats -- the last pixel needs no whole stride, and the host form copies exactly that much. */
#define SILENT_DT_U8 0
#define SILENT_DT_F32 1
#define SILENT_DT_F64 2
#define SILENT_DT_I32 3
#define SILENT_DT_U16 4
#define SILENT_DT_I16 5
#define SILENT_DT_I64 6
int silent_cast_interleave(silent_ctx* ctx, const void* in, int in_dtype, size_t n_pixels, int in_stride, int in_offset,
                           int count, float* out, int out_stride, int out_offset);
int silent_cast_interleave_dev(silent_ctx* ctx, const void* in, int in_dtype, size_t n_pixels, int in_stride, int in_offset,
                               int count, float* out, int out_stride, int out_offset, silent_stream stream);

/* tf.image.resize_nearest_neighbor with the TF1 defaults (align_corners = False), recognition_testing.py:82-83
 * and util/centroids.py:41: out(y, x) = in(min(floor(y * float32(in_h / out_h)), in_h - 1), ...).
 * in: packed maps with extents in_levels; out: packed maps with extents out_levels (same level count). */
int silent_resize_nearest(silent_ctx* ctx, const float* in, const silent_extent* in_levels, int n_levels,
                          int n_frames, int channels, const silent_extent* out_levels, float* out);
int silent_resize_nearest_dev(silent_ctx* ctx, const float* in, const silent_extent* in_levels, int n_levels,
                              int n_frames, int channels, const silent_extent* out_levels, float* out,
                              silent_stream stream);

/* ---------------------------------------------------------------------------- fused RGB chain
 * The reference graph recognition_testing.py:69-77 on 3-channel levels.  With a channel-uniform blur (what
 * blur_tensor generates) this is ONE fused launch that reads the pyramid once; any other blur runs the
 * stages as separate launches through workspace temporaries:
 *   orient   = regulate(relu(conv(relu(conv(relu(conv(x, rgc)), rgby)), stripe)), blur, rv, root)   (:69-71)
 *   line_end = pad_inwards(clip(relu(conv(orient, end)), 0, clip_hi), pad)                          (:73-75)
 *   value    = get_value_from_color(line_end)                                                        (:77)
 * Every kernel is HWIO [3,3,3,3] except blur [7,7,3,3].  Any of the three outputs may be NULL.
 * The regulator of the fused launch, m = min(blur sum, 1): rv * exp2(-root * log2(m)) for m >= 7.8886e-31 (just below
 * 2^-100), powf and a division below it (denormal sums included, none flushed) and for root = 0; within
 * (3 ln2 root |log2 m| + 8) * 2^-24 of |orient| of silent_regulate's definition for 0 <= root <= 1, which stays below 1e-5
 * (tests/test_gpu_regulator_domain.py).  The blur sum of a relu'd stripe map under non-negative blur weights is never
 * negative; for a negative sum the fused launch gives NaN for every root but 0, unlike silent_regulate at root 1. */
typedef struct silent_rgb_chain_params {
    const float* rgc;    /* midget_rgc(2)              filters/rgc.py:9      */
    const float* rgby;   /* rgby_3(2)                  filters/rgby.py:9     */
    const float* stripe; /* rgb_2d_stripe_tensors()    filters/orientation.py:19 */
    const float* blur;   /* blur_tensor(2, 7)          filters/orientation.py:20 */
    const float* end;    /* rgb_2d_end_tensors()       recognition_testing.py:29 */
    float regulation_value, regulation_root; /* 1.0, 0.1   filters/orientation.py:33 */
    int32_t flat_policy;
    float clip_hi;       /* 255                        recognition_testing.py:74 */
    int32_t pad;         /* 2                          recognition_testing.py:75 */
} silent_rgb_chain_params;

/* Host-only: which structure silent_rgb_line_end finds in the weights (no GPU needed).  flags: bit 0 rgc is
 * channel-diagonal, bit 1 stripe does not depend on the input channel, bit 2 rgby / bit 3 end are "two-group" kernels
 * (every tap vector K[t][i][:] a multiple of one of two vectors), bit 4 every channel of rgc is mirror-symmetric in both axes,
 * bit 5 rgby = S (x) A around the centre + B at the centre with a profile S that is mirror-symmetric in both axes.  masks (may
 * be NULL): 6 words, the group-A tap masks (bit dy * 3 + dx) of rgby and end per input channel. */
int silent_rgb_chain_structure(const silent_rgb_chain_params* params, unsigned* flags, unsigned* masks);

/* Config 3 from the pyramid on in ONE call (recognition_testing.py:69-77 followed by a-10 -> a-9 -> a-8 -> a-11 on its result):
 * = silent_rgb_line_end, then silent_select_keypoints(color = line_end, value = its value map, channels = 3).  Same outputs,
 * bit for bit, as those two calls.  The fused chain kernel accumulates the per-level max / min of the value map that a-10's
 * threshold needs (top_value_points.py:16-27) while it writes line_end, so the separate reduction pass and -- unless value_out
 * is given -- the value map itself are never moved through memory.  orient_out / value_out may be NULL; the host form also
 * accepts NULL line_end_out; idx / cap_per_frame / counts as silent_max_value_indices_region.
 * peak_value_out may be NULL (both forms): nobody then needs the selection's value map as a MAP.  Either way the tail runs sparse --
 * the chain kernel leaves max_pool(value) per (pixel pair x 16 rows), and a-10 / a-9 / a-8 / a-11 are evaluated only around
 * the pixels that reach their level's threshold (a handful per level on natural and noise frames).  A search window
 * without a positive peak makes every non-NaN pixel mapped to it a keypoint: in a level without NaNs (the chain kernel
 * notes them) the count pass synthesises that; with NaNs, or with > 16384 candidates in a frame, the (frame, level) runs
 * the dense kernels on a map in the context workspace.  With peak_value_out given, the map is zero-filled and receives the
 * evaluated pixels' values; levels that hold NaNs run the dense pass (a NaN pixel's peak value is a NaN).  Keypoints and map are
 * identical either way (tested). */
int silent_rgb_keypoints(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                         const silent_rgb_chain_params* params, double top_percent, const silent_extent* regions,
                         float* orient_out, float* line_end_out, float* value_out, float* peak_value_out, int64_t* idx,
                         size_t cap_per_frame, int64_t* counts);
int silent_rgb_keypoints_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                             const silent_rgb_chain_params* params, double top_percent, const silent_extent* regions,
                             float* orient_out, float* line_end_out, float* value_out, float* peak_value_out, int64_t* idx,
                             size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* BASELINE configs 1 / 2 / 5 with keypoints: silent_gray_pass (pyr, cs_out, end_out bit-identical to it for the same arguments;
 * end_out stays UNPADDED) followed by the reference graph's tail restricted to one input channel (recognition_testing.py:75-90)
 * on its K-channel end map: color = pad_inwards(end, pad), value = get_value_from_color(color), then
 *   selection = 1: top_value_points -> 3x3 NMS (product form) -> get_value_from_color -> max_value_indices_region, i.e.
 *                  silent_select_keypoints(color, value, channels = K); sparse like silent_rgb_keypoints (the kernels that write
 *                  `end` leave the per-level extrema, the value summary and NaN flags; SILENT_TUNE_GRAY bit 6 forces the dense kernels);
 *   selection = 0: max_value_indices_region on value (recognition_testing.py:90).
 * end_out is required (the keypoints are taken from it; the host form accepts NULL pyr / end_out), cs_out may be NULL;
 * value_out [1 ch] and peak_value_out [1 ch, selection = 1 only] may be NULL.  regions: one silent_extent per level of the plan.
 * idx / cap_per_frame / counts as silent_max_value_indices_region (the host form returns SILENT_E_CAPACITY, the _dev form leaves
 * the overflow in counts).  n_orient: 3, 4 or 8; pad >= 0.  silent_sparse_tail_stats reports on the last call. */
int silent_gray_keypoints(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out,
                          float* end_out, int pad, int selection, double top_percent, const silent_extent* regions,
                          float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts);
int silent_gray_keypoints_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                              const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                              float* cs_out, float* end_out, int pad, int selection, double top_percent,
                              const silent_extent* regions, float* value_out, float* peak_value_out, int64_t* idx,
                              size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* The same on uint8 frames (see silent_gray_pass_u8): every output is that of silent_gray_keypoints[_dev] given (float)frames[i]. */
int silent_gray_keypoints_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                             const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out,
                             float* end_out, int pad, int selection, double top_percent, const silent_extent* regions,
                             float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts);
int silent_gray_keypoints_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                 const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                 float* cs_out, float* end_out, int pad, int selection, double top_percent,
                                 const silent_extent* regions, float* value_out, float* peak_value_out, int64_t* idx,
                                 size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* The same on interleaved 3-channel uint8 frames [n, H, W, 3] (see silent_gray_pass_u8x3): every output is that of
 * silent_gray_keypoints[_dev] given the frame of values (b0 + b1 + b2) * float32(1/3). */
int silent_gray_keypoints_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                               const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out,
                               float* end_out, int pad, int selection, double top_percent, const silent_extent* regions,
                               float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts);
int silent_gray_keypoints_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                   const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                   float* cs_out, float* end_out, int pad, int selection, double top_percent,
                                   const silent_extent* regions, float* value_out, float* peak_value_out, int64_t* idx,
                                   size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* The same on a strided uint8 view (see silent_gray_pass_view): every output is that of silent_gray_keypoints_u8[_dev] /
 * silent_gray_keypoints_u8x3[_dev] on the compacted copy of the view's pixels. */
int silent_gray_keypoints_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                               const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out,
                               float* end_out, int pad, int selection, double top_percent, const silent_extent* regions,
                               float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts);
int silent_gray_keypoints_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                   const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                   float* cs_out, float* end_out, int pad, int selection, double top_percent,
                                   const silent_extent* regions, float* value_out, float* peak_value_out, int64_t* idx,
                                   size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* The same on uint16 frames (see silent_gray_pass_u16) and on a strided uint16 view (silent_gray_pass_view16): every output is that
 * of silent_gray_keypoints[_dev] on the widened frame / of silent_gray_keypoints_u16[_dev] on the compacted copy of the view's pixels. */
int silent_gray_keypoints_u16(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                              const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out,
                              float* end_out, int pad, int selection, double top_percent, const silent_extent* regions,
                              float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts);
int silent_gray_keypoints_u16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                                  const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                  float* cs_out, float* end_out, int pad, int selection, double top_percent,
                                  const silent_extent* regions, float* value_out, float* peak_value_out, int64_t* idx,
                                  size_t cap_per_frame, int64_t* counts, silent_stream stream);
int silent_gray_keypoints_view16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                 const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out,
                                 float* end_out, int pad, int selection, double top_percent, const silent_extent* regions,
                                 float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts);
int silent_gray_keypoints_view16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                     const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                     float* cs_out, float* end_out, int pad, int selection, double top_percent,
                                     const silent_extent* regions, float* value_out, float* peak_value_out, int64_t* idx,
                                     size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* What the sparse tail of the LAST silent_rgb_keypoints[_dev] / silent_gray_keypoints[_dev] call of this context did (synchronises that call's stream):
 * stats[0] = 1 if it ran sparse, [1] = (frame, level) pairs, [2] = pairs it handed to the dense kernels, [3] = candidate
 * pixels (value >= threshold) it evaluated, [4] = pairs settled with a synthesised all-zero map (a search window without a
 * positive peak in a level without NaNs: every pixel mapped to it is a keypoint).  stats holds 5 values.  For tests and the
 * bench report; no reference counterpart. */
int silent_sparse_tail_stats(silent_ctx* ctx, int64_t* stats);

/* Host-only (no GPU needed): the weight STREAM silent_rgb_line_end hands to its pair kernel for these weights -- the
 * weights in the order the kernel consumes them (csrc/silent_rgb2.h), zero-padded to whole pairs of 16-float blocks.
 * knobs: SILENT_TUNE_RGB bits 0 / 1 / 6.  variant: 3 symmetric forms (rgc folded over both mirror axes, rgby as channel mix ->
 * one profile -> centre mix, the stripe bank as left / right SGPR pairs), 2 two-group, 1 basic (diagonal rgc + channel-sum
 * stripe), 0 dense; n_used = 149 / 160 / 265 / 373 (two-group and symmetric: the mirror-symmetric blur travels as 16 folded
 * weights).  stream must hold SILENT_RGB_STREAM_MAX floats.  For tests of the host logic. */
#define SILENT_RGB_STREAM_MAX 384
int silent_rgb_chain_stream(const silent_rgb_chain_params* params, unsigned knobs, float* stream, int* n_used, int* variant);
int silent_rgb_line_end(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                        const silent_rgb_chain_params* params, float* orient_out, float* line_end_out,
                        float* value_out);
int silent_rgb_line_end_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                            int n_frames, const silent_rgb_chain_params* params, float* orient_out,
                            float* line_end_out, float* value_out, silent_stream stream);

/* FLOAT16 STORAGE of the orient and line_end maps: silent_rgb_line_end[_dev] with orient_out / line_end_out as IEEE binary16
 * (uint16_t bit patterns, 2-byte aligned, the same NHWC [.., h, w, 3] layout at 6 bytes per pixel).  All arithmetic is the float32
 * call's: the same kernel instantiation and tile height as silent_rgb_line_end with the same arguments and context tuning, and every
 * stored element is the float32 call's element rounded ONCE at the store -- to nearest even, overflow to +-inf (a clip_hi above 65504
 * can reach it), a NaN stays a NaN (payload unspecified), binary16 subnormals are kept.  value_out stays float32 and is bit-identical
 * to the float32 call's (it is taken from the unrounded line_end).  Half the bytes written and kept for the two colour maps.
 * RGB knob bits 4 (one-pixel kernel) and 7 (16-byte stores) are float32 store forms and are not honoured.  SILENT_E_UNSUPPORTED where
 * the float32 call would leave the pair kernel: a blur that is not channel-uniform (the stage-per-launch route), or a level too large
 * for that kernel's addressing.  Every other refusal is silent_rgb_line_end's. */
int silent_rgb_line_end_h(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                          const silent_rgb_chain_params* params, uint16_t* orient_out, uint16_t* line_end_out,
                          float* value_out);
int silent_rgb_line_end_h_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                              int n_frames, const silent_rgb_chain_params* params, uint16_t* orient_out,
                              uint16_t* line_end_out, float* value_out, silent_stream stream);

/* silent_rgb_keypoints[_dev] with float16 orient / line_end maps:
 * = silent_rgb_line_end_h, then silent_select_keypoints(color = (float)line_end_h, value = the FLOAT32 value map, channels = 3):
 * idx, counts and peak_value_out equal that pair of calls bit for bit; the maps are silent_rgb_line_end_h's.  line_end_out is
 * required in both forms (the tail reads it; it widens each element where it loads it).  The threshold (the value map's per-level
 * extrema) and the set of pixels that pass it come from the float32 value map and are those of silent_rgb_keypoints.  The
 * keypoints themselves can differ from silent_rgb_keypoints' where rounding makes or breaks a TIE: the 3x3 non-maximum suppression
 * compares a rounded colour with the rounded maximum of its neighbourhood, and a region's keypoints are the pixels that reach its
 * rounded maximum -- two float32 values that differ below binary16's resolution become equal.  Refusals as silent_rgb_keypoints,
 * and SILENT_E_UNSUPPORTED as silent_rgb_line_end_h. */
int silent_rgb_keypoints_h(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                           const silent_rgb_chain_params* params, double top_percent, const silent_extent* regions,
                           uint16_t* orient_out, uint16_t* line_end_out, float* value_out, float* peak_value_out, int64_t* idx,
                           size_t cap_per_frame, int64_t* counts);
int silent_rgb_keypoints_h_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                               const silent_rgb_chain_params* params, double top_percent, const silent_extent* regions,
                               uint16_t* orient_out, uint16_t* line_end_out, float* value_out, float* peak_value_out, int64_t* idx,
                               size_t cap_per_frame, int64_t* counts, silent_stream stream);

/* ---------------------------------------------------------------------------- one camera frame, one call
 * LineEndDisplayer.callback + run, slam_recognition/recognition_testing.py:106-144: a frame in host memory ->
 * np.asarray(frame, float32) (:141) -> zoom.from_image(frame, 3, output_size, zoom_ratio) (:142) -> the graph of compile()
 * (:60-100) -> the six tensors session.run fetches (:99-100, :132), in host memory:
 *   0 orient [L,h,w,3]   1 255 - centroids * 255 [L,h,w,1]   2 255 - centroids2 * 255 [L,h2,w2,1] (h2 = int(h / e ** .5))
 *   3 fired * 255 [L,ch,cw,C]   4 update_importances [L,ch,cw,C]   5 padded line_end [L,h,w,3]      (ch = ceil(h / region_h);
 *                                                                                      C = 3 with boosting.visualize, else 1)
 * The reference pays a feed, a session.run and six fetches per frame; the displayer replays ONE HIP graph per frame (five kernels
 * that read the pinned input buffer and write the pinned result slot themselves: no copy node) on a stream of its own and owns every buffer, a private context and the boosting state
 * (energy_values, :56; 8 everywhere at creation).  levels: the host's geometry of image_to_zoom_tensor (from_image.py:45-64),
 * every level on the same canvas extent.  Not thread-safe; frames of one camera must come to one displayer, in order. */
typedef struct silent_displayer silent_displayer;
typedef struct silent_displayer_params {
    int32_t frame_h, frame_w;        /* camera frame [frame_h, frame_w, 3] */
    int32_t frame_dtype;             /* SILENT_DT_U8 (a camera's) ... SILENT_DT_F32 */
    int32_t centroid_region_h, centroid_region_w;   /* centroid_region_shape[1:3] = 3, 3 (recognition_testing.py:38) */
    silent_rgb_chain_params chain;   /* kernels are copied at creation */
    silent_boosting_params boosting; /* get_boosting(..., 1, 1, recovery, True): visualize = 1 in the reference (:86) */
} silent_displayer_params;
int silent_displayer_create(silent_ctx* ctx, const silent_displayer_params* params, const silent_pyr_level* levels, int n_levels,
                            silent_displayer** out);
/* Lifetime: `ctx` (errors of the displayer's calls are reported there) must outlive every silent_displayer_step / _input /
 * _get_state / _set_state call; silent_displayer_destroy itself does not touch it (it may run after silent_destroy(ctx), e.g. at
 * interpreter shutdown).  destroy frees the pinned input buffer and both result slots: pointers handed out by _step / _input die
 * with it. */
void silent_displayer_destroy(silent_displayer* d);
/* shape7 = {L, h, w, ch, cw, h2, w2}; out_floats6 (may be NULL): floats of each of the six results */
int silent_displayer_shape(const silent_displayer* d, int32_t* shape7, size_t* out_floats6);
/* Synchronous.  results[0..5]: pointers INTO the displayer's pinned result slot, valid until the SECOND next step (two slots
 * alternate).  gpu_ms (may be NULL): device time of the frame from HIP events around the graph; the call then ends in a stream
 * synchronisation.  With gpu_ms == NULL it waits for the frame's own completion word instead -- a one-thread kernel behind the last
 * one stores the frame count into pinned host memory, the host polls it (bounded: after 20 ms it synchronises the stream the
 * ordinary way, where a failed launch surfaces) -- which is ~0.02 ms less wall time per frame. */
int silent_displayer_step(silent_displayer* d, const void* frame_host, const float** results, float* gpu_ms);
/* More result slots, for callers that hand the results out zero-copy and must not overwrite what somebody still holds (the reference's
 * session.run returns fresh arrays, recognition_testing.py:132): silent_displayer_add_slot allocates one more pinned slot (numbers 0 and
 * 1 exist from creation: silent_displayer_step alternates between those two), silent_displayer_step_slot is silent_displayer_step
 * into a slot of the caller's choice -- one nobody references any more (pysilent_amd._runtime.FrameDisplayer keeps the books). */
int silent_displayer_add_slot(silent_displayer* d, int* slot_index);
int silent_displayer_step_slot(silent_displayer* d, const void* frame_host, int slot, const float** results, float* gpu_ms);
/* The displayer's pinned input buffer: a capture loop that writes the camera frame THERE and passes this pointer to
 * silent_displayer_step skips the staging copy (6 MB per 1080p frame).  A frame_host that overlaps the buffer at another
 * offset is moved into place (memmove). */
int silent_displayer_input(silent_displayer* d, void** frame_buffer, size_t* bytes);
int silent_displayer_get_state(silent_displayer* d, float* energy_host);       /* [L, ch, cw] */
int silent_displayer_set_state(silent_displayer* d, const float* energy_host);

/* ---------------------------------------------------------------------------- the same tail for a batch of streams
 * What LineEndDisplayer.compile computes after the line-end map (recognition_testing.py:77-100), on a PACKED pyramid batch: every frame
 * slot is a camera stream of its own, every level has its own extents.  value: packed 1-channel maps, the layout of
 * silent_rgb_line_end's value_out (get_value_from_color(pad_inwards(line_end))).  Results and the advanced state are those of this
 * sequence of the entry points above on the same value, BIT FOR BIT, NaNs included (an empty cell gives 0 / 0):
 *     g      = affine_clip(value, div = 255)                   dist,  tot = centroids(g, region_h, region_w)
 *     imp    = affine_clip(tot, 255 / 4, 0, 1, 256, -1)        im2        = resize_nearest(value, half)
 *     dist2, _ = centroids(affine_clip(im2, div = 255), ...)   fired, upd = boosting_step(imp, energy, boosting)
 *     centroids_out = affine_clip(dist, -255, 255)     centroids2_out = affine_clip(dist2, -255, 255)
 *     fired_out     = affine_clip(fired, 255)          update_out     = upd
 * in two launches, with no intermediate map in memory (8 + 8 + 4 + 4 bytes per cell of workspace).
 *   energy          caller-owned state [n_frames][cells of every level], updated in place (the contract of silent_boosting_step)
 *   centroids_out   255 - dist * 255, laid out like value
 *   centroids2_out  the same on the nearest-neighbour half map: level l has (int)((float)h / resize_div) x (int)((float)w / resize_div)
 *                   pixels (float32 division, truncated: recognition_testing.py:82-83), packed with those extents
 *   fired_out       fired * 255, update_out: update_importances; packed with the cell extents (level l: ceil(h / region_h) x
 *                   ceil(w / region_w)), 3 channels when boosting.visualize is set, else 1
 * Any of the four outputs may be NULL; with centroids2_out == NULL nothing of the half map is computed.  SILENT_E_INVALID: NULL value,
 * energy or params; n_levels outside 1 .. SILENT_MAX_LEVELS; n_frames < 1; a region extent below 1; a non-positive level extent;
 * resize_div below 1 or not finite; a level whose half extent would be 0.
 * silent_attention_extents: host only, no GPU work and no context (its message: silent_last_error(NULL)): per level the cell extents
 * of the map, the half extents, the cell extents of the half map; each output may be NULL. */
typedef struct silent_attention_params {
    int32_t region_h, region_w;        /* centroid_region_shape[1:3] = 3, 3 (recognition_testing.py:39) */
    float resize_div;                  /* float32(e ** .5) (:82-83) */
    silent_boosting_params boosting;   /* as silent_boosting_step takes them */
} silent_attention_params;

int silent_attention_extents(const silent_extent* levels, int n_levels, const silent_attention_params* params, silent_extent* cells,
                             silent_extent* half, silent_extent* cells2);
int silent_attention_tail(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels, int n_frames,
                          const silent_attention_params* params, float* energy, float* centroids_out, float* centroids2_out,
                          float* fired_out, float* update_out);
int silent_attention_tail_dev(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels, int n_frames,
                              const silent_attention_params* params, float* energy, float* centroids_out, float* centroids2_out,
                              float* fired_out, float* update_out, silent_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SILENT_HIP_H */
