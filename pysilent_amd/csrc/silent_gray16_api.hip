// libsilent_hip.so -- the grayscale pass on uint16 frames (silent_gray_pass.h): the *_u16 and *_view16 entry points of the pass and
// the instantiations of its frame-reading kernels for the two uint16 frame kinds.
#include "silent_gray_pass.h"

#define X(FT)                                                                                                                        \
    template int gray_pass_kp<FT>(silent_ctx*, const silent_pyramid_plan*, const FT*, int, const float*, const float*, int, float, float*, \
                                  float*, float*, const GrayKp&, hipStream_t);
SILENT_FRAME_TYPES_16(X)
#undef X

// uint16 frames (silent_hip.h): the *_u8 forms with an unsigned 16-bit element, 2-byte aligned.
SILENT_EXPORT int silent_gray_pass_u16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                                           const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                           void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    TRY(check_u16_aligned(ctx, "silent_gray_pass_u16", frames));
    return gray_pass_maps(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u16_dev");
}

SILENT_EXPORT int silent_gray_pass_u16(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                                       const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                       void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    TRY(check_u16_aligned(ctx, "silent_gray_pass_u16", frames));
    return gray_pass_host(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u16");
}

// Strided uint16 views: the view's own refusals and those of the *_u16 form under the view's name, then the frame kind that reads it
// (with_view16: a packed view takes the packed kernels).
static int gray_pass_view16(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const silent_frame_view16* view, int n_frames,
                            const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out, void* end_out,
                            bool f16, unsigned parts, silent_stream stream) {
    const char* who = "silent_gray_pass_view16";
    TRY(check_view16(ctx, who, plan, view, n_frames, nullptr));
    TRY(gray_pass_checks<View16>(ctx, who, plan, true, n_frames, cs_kernel, end_bank, n_orient, pyr, cs_out, end_out, f16, parts));
    return with_view16(plan, view, n_frames, [&](auto frames) {
        if (host) return gray_pass_host(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, f16);
        return gray_pass_maps(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, f16, parts, stream);
    });
}

SILENT_EXPORT int silent_gray_pass_view16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                              const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                              void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_view16(ctx, false, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, parts,
                            stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_view16_dev");
}

SILENT_EXPORT int silent_gray_pass_view16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                          void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    return gray_pass_view16(ctx, true, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, 3u,
                            nullptr);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_view16");
}
