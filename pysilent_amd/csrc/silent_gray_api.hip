// libsilent_hip.so -- the grayscale pass (silent_gray.h): CS -> line-end bank on a pyramid, and the whole pass from the frame
// (pyramid + unit levels in one read of the frame, then the remaining levels) on float and uint8 frames.  The bodies every frame kind
// shares are in silent_gray_pass.h; the uint16 kinds' entry points and kernels are a unit of their own, silent_gray16_api.hip.
#include "silent_gray_pass.h"

// ------------------------------------------------------------------------------------------ fused gray pass

// ST: the element type of the CS and end maps -- float, or gray_half (float16 storage: silent_gray_pass_h); FT: the frame element type
// -- float, unsigned char (the *_u8 entry points) or FrameRgb8 (the *_u8x3 entry points, silent_common.h).  Which kernels exist for
// them, and how (kp, f64, n_orient, the plan's stream layout) become template arguments: kGrayKernel, with_gray_mode, with_orient,
// with_stream_layout (silent_plan.h).  f64: the F64 kernel (F64 plans only, silent_gray_line_end always runs float32).
template <typename ST>
int launch_gray(silent_ctx* ctx, const char* who, const float* pyr, const silent_extent* levels, int n_levels,
                int n_frames, const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi,
                ST* cs_out, ST* end_out, hipStream_t s, const bool* skip, const GrayKp* kp, bool f64) {
    if (!pyr || !cs_kernel) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    TRY(check_gray_outputs(ctx, who, cs_out, end_out, end_bank, n_orient));
    // development knob for interleaved A/B timing (scripts/ab_gray.py): bit0 XCD-aware tile order (measured
    // 7 % slower, off), bit2 non-temporal stores (no effect, off).  (Bit1 selected 32-row tiles until round 5: 3 % slower in every
    // A/B and 145 - 156 SGPR spills; the instantiations are gone since round 6, the bit is ignored.)
    const unsigned opts = ctx->tune[SILENT_TUNE_GRAY];
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kGrayTW, kGrayTH, &tab, &blocks, skip));
    if (blocks == 0) return SILENT_OK;
    const GrayW w = gray_weights(cs_kernel, end_bank, n_orient);
    with_orient(n_orient, [&](auto K) {
        with_gray_mode<ST, float>(kp != nullptr, f64, [&](auto KP, auto F64) {
#define LINE_END(...) \
    hipLaunchKernelGGL((gray_line_end_kernel<decltype(K)::value, kGrayTH, decltype(KP)::value, decltype(F64)::value, ST>), \
                       dim3((unsigned)blocks), dim3(256), 0, s, pyr, cs_out, end_out, tab, w, clip_hi, opts, ##__VA_ARGS__)
            if constexpr (decltype(KP)::value) LINE_END(*kp);
            else LINE_END();
#undef LINE_END
        });
    });
    return check_launch(ctx, who);
}

template int launch_gray<float>(silent_ctx*, const char*, const float*, const silent_extent*, int, int, const float*, const float*, int, float, float*,
                                float*, hipStream_t, const bool*, const GrayKp*, bool);
template int launch_gray<gray_half>(silent_ctx*, const char*, const float*, const silent_extent*, int, int, const float*, const float*, int, float,
                                    gray_half*, gray_half*, hipStream_t, const bool*, const GrayKp*, bool);

SILENT_EXPORT int silent_gray_line_end_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels,
                                           int n_levels, int n_frames, const float* cs_kernel, const float* end_bank,
                                           int n_orient, float clip_hi, float* cs_out, float* end_out,
                                           silent_stream stream) try {
    NEED_CTX(ctx);
    return launch_gray(ctx, "silent_gray_line_end", pyr, levels, n_levels, n_frames, cs_kernel, end_bank, n_orient,
                       clip_hi, cs_out, end_out, (hipStream_t)stream, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_gray_line_end_dev");
}

// (the uint16 kinds: silent_gray16_api.hip)
#define X(FT)                                                                                                                        \
    template int gray_pass_kp<FT>(silent_ctx*, const silent_pyramid_plan*, const FT*, int, const float*, const float*, int, float, float*, \
                                  float*, float*, const GrayKp&, hipStream_t);
SILENT_FRAME_TYPES_8(X)
#undef X

SILENT_EXPORT int silent_gray_pass_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames,
                                       int n_frames, const float* cs_kernel, const float* end_bank, int n_orient,
                                       float clip_hi, float* pyr, float* cs_out, float* end_out,
                                       silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, 3u, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_dev");
}

SILENT_EXPORT int silent_gray_pass_parts_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames,
                                             int n_frames, const float* cs_kernel, const float* end_bank, int n_orient,
                                             float clip_hi, float* pyr, float* cs_out, float* end_out, unsigned parts,
                                             silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_parts_dev");
}

SILENT_EXPORT int silent_gray_line_end(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                                       int n_frames, const float* cs_kernel, const float* end_bank, int n_orient,
                                       float clip_hi, float* cs_out, float* end_out) try {
    NEED_CTX(ctx);
    const char* who = "silent_gray_line_end";
    if (!pyr || !cs_kernel) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    TRY(check_gray_outputs(ctx, who, cs_out, end_out, end_bank, n_orient));
    long long px;
    TRY(check_levels(ctx, who, levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t b1 = (size_t)px * 4;
    const int x = hs.in(pyr, b1), cs = hs.out(cs_out, b1), end = hs.out(end_out, b1 * n_orient);
    return hs.run([&] {
        return silent_gray_line_end_dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, cs_kernel, end_bank, n_orient, clip_hi,
                                        hs.dev<float>(cs), hs.dev<float>(end), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_gray_line_end");
}

SILENT_EXPORT int silent_gray_pass(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                                   const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi,
                                   float* pyr, float* cs_out, float* end_out) try {
    NEED_CTX(ctx);
    return gray_pass_host(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, false);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass");
}

SILENT_EXPORT int silent_gray_pass_h_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                                         const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                         uint16_t* cs_out, uint16_t* end_out, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_maps(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, true, parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_h_dev");
}

SILENT_EXPORT int silent_gray_pass_h(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                                     const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                     uint16_t* cs_out, uint16_t* end_out) try {
    NEED_CTX(ctx);
    return gray_pass_host(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, true);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_h");
}

SILENT_EXPORT int silent_gray_pass_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                          void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_maps(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8_dev");
}

SILENT_EXPORT int silent_gray_pass_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                      const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                      void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    return gray_pass_host(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8");
}

SILENT_EXPORT int silent_gray_pass_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                            const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                            void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_maps(ctx, plan, rgb8(frames), n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, parts,
                          stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8x3_dev");
}

SILENT_EXPORT int silent_gray_pass_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                        const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                        void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    return gray_pass_host(ctx, plan, rgb8(frames), n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8x3");
}

// Strided uint8 views (silent_hip.h): the view's own refusals and those of the *_u8 form under the view's name, then the frame kind
// that reads it (with_view: a packed view takes the packed kernels).
static int gray_pass_view(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const silent_frame_view* view, int n_frames,
                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out, void* end_out,
                          bool f16, unsigned parts, silent_stream stream) {
    const char* who = "silent_gray_pass_view";
    TRY(check_view(ctx, who, plan, view, n_frames, nullptr));
    TRY(gray_pass_checks<View8>(ctx, who, plan, true, n_frames, cs_kernel, end_bank, n_orient, pyr, cs_out, end_out, f16, parts));
    return with_view(plan, view, n_frames, [&](auto frames) {
        if (host) return gray_pass_host(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, f16);
        return gray_pass_maps(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, f16, parts, stream);
    });
}

SILENT_EXPORT int silent_gray_pass_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                            const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                            void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_view(ctx, false, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, parts,
                          stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_view_dev");
}

SILENT_EXPORT int silent_gray_pass_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                        const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                        void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    return gray_pass_view(ctx, true, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, maps_f16 != 0, 3u,
                          nullptr);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_view");
}
