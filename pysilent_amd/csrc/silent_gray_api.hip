// libsilent_hip.so -- the grayscale pass (silent_gray.h): CS -> line-end bank on a pyramid, and the whole pass from the frame
// (pyramid + unit levels in one read of the frame, then the remaining levels).
#include "silent_plan.h"

using namespace silent;

// ------------------------------------------------------------------------------------------ fused gray pass

// ST: the element type of the CS and end maps -- float, or gray_half (float16 storage: silent_gray_pass_h); FT: the frame element type
// -- float, unsigned char (the *_u8 entry points) or FrameRgb8 (the *_u8x3 entry points, silent_common.h).  Which kernels exist for
// them, and how (kp, f64, n_orient, the plan's stream layout) become template arguments: kGrayKernel, with_gray_mode, with_orient,
// with_stream_layout (silent_plan.h).  f64: the F64 kernel (F64 plans only, silent_gray_line_end always runs float32).
template <typename ST>
static int launch_gray(silent_ctx* ctx, const char* who, const float* pyr, const silent_extent* levels, int n_levels,
                       int n_frames, const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi,
                       ST* cs_out, ST* end_out, hipStream_t s, const bool* skip, const GrayKp* kp = nullptr, bool f64 = false) {
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

// everything silent_gray_pass*_dev refuses, before a launch (and, in the host forms, before the batch is staged); FT: the frame kind of
// the ENTRY POINT (the view entry points check as a strided kind whatever kind then reads the view), has_frames: its frames are not NULL
template <typename FT>
static int gray_pass_checks(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, bool has_frames, int n_frames,
                            const float* cs_kernel, const float* end_bank, int n_orient, const float* pyr, const void* cs_out,
                            const void* end_out, bool f16, unsigned parts) {
    if (!plan || !has_frames || !pyr || !cs_kernel) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (plan->ctx != ctx) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": plan belongs to another context");
    if constexpr (kFrameNarrow<FT>) TRY(check_narrow_frames(ctx, who, plan));
    if (f16) TRY(check_half_storage(ctx, who, plan));
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": the plan must be single-channel");
    TRY(check_gray_outputs(ctx, who, cs_out, end_out, end_bank, n_orient));
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_frames must be >= 1");
    if (!(parts & 3u)) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": parts must name step 1 + 2 (bit 0) and / or step 3 (bit 1)");
    return SILENT_OK;
}

// parts: bit 0 = the pyramid of every level + CS / end of the unit levels (steps 1 and 2), bit 1 = CS + end of the remaining levels
// (step 3, which reads the pyramid steps 1 and 2 wrote)
template <typename ST, typename FT>
static int gray_pass_parts(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames,
                           const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                           ST* cs_out, ST* end_out, unsigned parts, silent_stream stream, const GrayKp* kp = nullptr) {
    const char* who = entry_name<FT>(kp ? kGrayKeypoints : kStoreHalf<ST> ? kGrayPassH : kGrayPass);
    TRY(gray_pass_checks<FT>(ctx, who, plan, frames != nullptr, n_frames, cs_kernel, end_bank, n_orient, pyr, cs_out, end_out, kStoreHalf<ST>, parts));
    hipStream_t s = (hipStream_t)stream;
    const PyrTab& pt = plan->tab;
    const int kopts = (int)ctx->tune[SILENT_TUNE_GRAY];  // A/B knob: bit4 disables the stream path (bit3, 32-row fused tiles, is ignored since round 6)
    const bool stream_path = plan->stream_ok && !(kopts & 16);
    // 1. non-unit levels of the pyramid: by the region kernel, unless the stream kernel of step 2 produces them
    //    from the same single read of the frame; plus the zero fill of canvases larger than their zoomed crop
    if (parts & 1u) TRY(launch_pyramid(ctx, who, plan, frames, n_frames, pyr, s, false, !stream_path));
    // 2. unit levels: pyramid + CS + end in one kernel
    FusedTab64 ft = fused_tab(plan);   // (the float32 kernels take its FusedTab part)
    bool is_unit[kMaxLevels] = {false};
    long long unit_px = 0;
    GrayKp kpu{};   // the unit levels' plan level numbers travel with the keypoint epilogue's arguments
    if (kp) kpu = *kp;
    for (int l = 0; l < pt.n_levels; ++l) {
        if (pt.lv[l].kind != kPyrUnit) continue;
        is_unit[l] = true;
        if (kp) kpu.level[ft.n] = l;
        fused_add_level(ft, pt, l);
        unit_px += (long long)pt.lv[l].out_h * pt.lv[l].out_w;
    }
    const long long blocks = (long long)ft.tiles_per_frame * n_frames;
    if (blocks > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many tiles for one launch");
    if (blocks && (parts & 1u)) {
        const GrayW w = gray_weights(cs_kernel, end_bank, n_orient);
        ctx->prof_sample = ctx->profiling && (ctx->prof_calls++ % ctx->prof_period) == 0;
        const int prof_slot = ctx->prof_recorded % silent_ctx::kProfPairs;
        if (ctx->prof_sample) HIP_TRY(ctx, hipEventRecord(ctx->prof_ev[prof_slot][0], s));
        with_orient(n_orient, [&](auto K) {
            with_gray_mode<ST, FT>(kp != nullptr, plan->f64, [&](auto KP, auto F64) {
                constexpr int k = decltype(K)::value;
                constexpr bool with_kp = decltype(KP)::value, f64 = decltype(F64)::value;
                const FusedTabT<f64>& t = ft;
                const dim3 grid((unsigned)blocks), block(64 * kFusedWaves);
                if (stream_path) {
                    const StreamTab& st = plan->stream;
                    const unsigned sopts = (unsigned)((kopts >> 5) & 1);
                    with_stream_layout(plan, [&](auto G, auto L) {
#define STREAM(...) \
    hipLaunchKernelGGL((gray_stream_kernel<k, decltype(G)::value, decltype(L)::value, with_kp, f64, ST, FT>), grid, block, 0, s, kernel_frames(frames), \
                       pyr, cs_out, end_out, t, st, w, clip_hi, sopts, ##__VA_ARGS__)
                        if constexpr (with_kp) STREAM(kpu);
                        else STREAM();
#undef STREAM
                    });
                } else {
#define FUSED(...) \
    hipLaunchKernelGGL((gray_unit_fused_kernel<k, kFusedTH, with_kp, f64, ST, FT>), grid, block, 0, s, kernel_frames(frames), pyr, cs_out, end_out, \
                       t, w, clip_hi, ##__VA_ARGS__)
                    if constexpr (with_kp) FUSED(kpu);
                    else FUSED();
#undef FUSED
                }
            });
        });
        if (ctx->prof_sample) {
            HIP_TRY(ctx, hipEventRecord(ctx->prof_ev[prof_slot][1], s));
            ++ctx->prof_recorded;
            ctx->prof_pixels = unit_px * n_frames;
        }
        TRY(check_launch(ctx, who));
    }
    // 3. CS + end on the remaining levels (they read the pyramid written in step 1)
    if (pt.n_general && (parts & 2u))
        TRY(launch_gray(ctx, who, pyr, plan->extents.data(), pt.n_levels, n_frames, cs_kernel, end_bank, n_orient,
                        clip_hi, cs_out, end_out, s, is_unit, kp, plan->f64));
    return SILENT_OK;
}

// silent_gray_keypoints*_dev (silent_peaks_api.hip): the whole pass with the keypoint epilogue in every kernel that writes `end`
template <typename FT>
int gray_pass_kp(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, const float* cs_kernel,
                 const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out, float* end_out, const GrayKp& kp,
                 hipStream_t s) {
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, 3u,
                           (silent_stream)s, &kp);
}
#define X(FT)                                                                                                                        \
    template int gray_pass_kp<FT>(silent_ctx*, const silent_pyramid_plan*, const FT*, int, const float*, const float*, int, float, float*, \
                                  float*, float*, const GrayKp&, hipStream_t);
SILENT_FRAME_TYPES(X)
#undef X

// The entry points of the pass: the maps as the ABI passes them (void*; f16: IEEE binary16, the ST = gray_half kernels -- uint16_t
// in the C ABI, plain C has no half type) on any frame type.  Every output of the uint8 kinds is the float32-frame entry point's,
// bit for bit (silent_hip.h has the contracts): a byte is widened in a register at the load, an interleaved colour pixel becomes
// (b0 + b1 + b2) * float32(1/3) there -- the plan is single-channel, the layout belongs to the call.
template <typename FT>
static int gray_pass_maps(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, const float* cs_kernel,
                          const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out, void* end_out, bool f16,
                          unsigned parts, silent_stream stream) {
    if (f16)
        return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr,
                               static_cast<gray_half*>(cs_out), static_cast<gray_half*>(end_out), parts, stream);
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, static_cast<float*>(cs_out),
                           static_cast<float*>(end_out), parts, stream);
}

// the host-pointer forms: the frames are staged as they are (frame_px_bytes each pixel), the maps in their storage's element size
template <typename FT>
static int gray_pass_host(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, const float* cs_kernel,
                          const float* end_bank, int n_orient, float clip_hi, float* pyr, void* cs_out, void* end_out, bool f16) {
    TRY(gray_pass_checks<FT>(ctx, entry_name<FT>(f16 ? kGrayPassH : kGrayPass), plan, frames != nullptr, n_frames, cs_kernel, end_bank, n_orient, pyr,
                         cs_out, end_out, f16, 3u));
    HostStage hs(ctx);
    const size_t px = (size_t)plan->tab.frame_px_out * n_frames, eb = f16 ? 2 : 4;
    const int x = hs.in(frames_host(frames), frames_bytes(plan, frames, n_frames)), p = hs.out(pyr, px * 4),
              cs = hs.out(cs_out, px * eb), end = hs.out(end_out, px * eb * n_orient);
    return hs.run([&] {
        const StagedFrames<FT> staged(frames, hs.dev<char>(x));
        return gray_pass_maps(ctx, plan, staged.p, n_frames, cs_kernel, end_bank, n_orient, clip_hi, hs.dev<float>(p), hs.dev<char>(cs),
                              hs.dev<char>(end), f16, 3u, nullptr);
    });
}

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
