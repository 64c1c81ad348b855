// libsilent_hip.so -- the grayscale pass (silent_gray.h): CS -> line-end bank on a pyramid, and the whole pass from the frame
// (pyramid + unit levels in one read of the frame, then the remaining levels).
#include "silent_plan.h"

using namespace silent;

// ------------------------------------------------------------------------------------------ fused gray pass

// ST: the element type of the CS and end maps -- float, or gray_half (float16 storage: silent_gray_pass_h).  The gray_half kernels
// exist without keypoint epilogue and without float64 accumulation only (both are refused before a launch), so those template
// combinations are never instantiated.
// f64: the F64 kernel (float64 accumulation; F64 plans only, silent_gray_line_end always runs float32)
template <int K, bool F64, typename ST>
static void launch_line_end(long long blocks, hipStream_t s, const float* pyr, ST* cs_out, ST* end_out, const LevelTab& tab,
                            const GrayW& w, float clip_hi, unsigned opts, const GrayKp* kp) {
    if constexpr (kStoreHalf<ST>) {
        hipLaunchKernelGGL((gray_line_end_kernel<K, kGrayTH, false, false, ST>), dim3((unsigned)blocks), dim3(256), 0, s, pyr, cs_out,
                           end_out, tab, w, clip_hi, opts);
    } else {
    if (kp)
        hipLaunchKernelGGL((gray_line_end_kernel<K, kGrayTH, true, F64>), dim3((unsigned)blocks), dim3(256), 0, s, pyr, cs_out, end_out,
                           tab, w, clip_hi, opts, *kp);
    else
        hipLaunchKernelGGL((gray_line_end_kernel<K, kGrayTH, false, F64>), dim3((unsigned)blocks), dim3(256), 0, s, pyr, cs_out, end_out,
                           tab, w, clip_hi, opts);
    }
}

template <typename ST>
static int launch_gray(silent_ctx* ctx, const char* who, const float* pyr, const silent_extent* levels, int n_levels,
                       int n_frames, const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi,
                       ST* cs_out, ST* end_out, hipStream_t s, const bool* skip, const GrayKp* kp = nullptr, bool f64 = false) {
    if (!pyr || !cs_kernel) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (!cs_out && !end_out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": both outputs are NULL");
    if (end_out && !end_bank) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": end_bank is NULL");
    if (n_orient != 3 && n_orient != 4 && n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": n_orient must be 3, 4 or 8");
    // development knob for interleaved A/B timing (scripts/ab_gray.py): bit0 XCD-aware tile order (measured
    // 7 % slower, off), bit2 non-temporal stores (no effect, off).  (Bit1 selected 32-row tiles until round 5: 3 % slower in every
    // A/B and 145 - 156 SGPR spills; the instantiations are gone since round 6, the bit is ignored.)
    const unsigned opts = ctx->tune[SILENT_TUNE_GRAY];
    const int th = kGrayTH;
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kGrayTW, th, &tab, &blocks, skip));
    if (blocks == 0) return SILENT_OK;
    GrayW w;
    std::memset(&w, 0, sizeof(w));
    std::memcpy(w.cs, cs_kernel, sizeof(float) * 9);
    if (end_bank) std::memcpy(w.end, end_bank, sizeof(float) * 9 * n_orient);
#define GRAY_LAUNCH(K_)                                                                   \
    if constexpr (kStoreHalf<ST>) launch_line_end<K_, false, ST>(blocks, s, pyr, cs_out, end_out, tab, w, clip_hi, opts, nullptr); \
    else if (f64) launch_line_end<K_, true, ST>(blocks, s, pyr, cs_out, end_out, tab, w, clip_hi, opts, kp); \
    else launch_line_end<K_, false, ST>(blocks, s, pyr, cs_out, end_out, tab, w, clip_hi, opts, kp)
    if (n_orient == 3) { GRAY_LAUNCH(3); }
    else if (n_orient == 4) { GRAY_LAUNCH(4); }
    else { GRAY_LAUNCH(8); }
#undef GRAY_LAUNCH
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

// FT: the frame element type -- float, unsigned char (uint8 frames: the *_u8 entry points) or FrameRgb8 (interleaved uint8 colour: the
// *_u8x3 entry points, silent_common.h).  The uint8 kernels of both kinds exist with float32
// accumulation only (F64 plans are refused before a launch), with and without keypoint epilogue, for both map storages.
template <int K, int G, int L, bool F64, typename ST, typename FT>
static void launch_stream(long long blocks, hipStream_t s, const FT* frames, float* pyr, ST* cs_out, ST* end_out,
                          const FusedTab64& ft, const StreamTab& st, const GrayW& w, float clip_hi, unsigned opts, const GrayKp* kp) {
    const FusedTabT<F64>& t = ft;
    if constexpr (kStoreHalf<ST>)
        hipLaunchKernelGGL((gray_stream_kernel<K, G, L, false, false, ST, FT>), dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s, frames,
                           pyr, cs_out, end_out, t, st, w, clip_hi, opts);
    else if (kp)
        hipLaunchKernelGGL((gray_stream_kernel<K, G, L, true, F64, ST, FT>), dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s, frames, pyr,
                           cs_out, end_out, t, st, w, clip_hi, opts, *kp);
    else
        hipLaunchKernelGGL((gray_stream_kernel<K, G, L, false, F64, ST, FT>), dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s, frames, pyr,
                           cs_out, end_out, t, st, w, clip_hi, opts);
}

template <int K, bool F64, typename ST, typename FT>
static void launch_fused(long long blocks, hipStream_t s, const FT* frames, float* pyr, ST* cs_out, ST* end_out,
                         const FusedTab64& ft, const GrayW& w, float clip_hi, const GrayKp* kp) {
    const FusedTabT<F64>& t = ft;
    if constexpr (kStoreHalf<ST>)
        hipLaunchKernelGGL((gray_unit_fused_kernel<K, kFusedTH, false, false, ST, FT>), dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s,
                           frames, pyr, cs_out, end_out, t, w, clip_hi);
    else if (kp)
        hipLaunchKernelGGL((gray_unit_fused_kernel<K, kFusedTH, true, F64, ST, FT>), dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s,
                           frames, pyr, cs_out, end_out, t, w, clip_hi, *kp);
    else
        hipLaunchKernelGGL((gray_unit_fused_kernel<K, kFusedTH, false, F64, ST, FT>), dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s,
                           frames, pyr, cs_out, end_out, t, w, clip_hi);
}

// parts: bit 0 = the pyramid of every level + CS / end of the unit levels (steps 1 and 2), bit 1 = CS + end of the remaining levels
// (step 3, which reads the pyramid steps 1 and 2 wrote)
template <typename ST, typename FT>
static int gray_pass_parts(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames,
                           const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                           ST* cs_out, ST* end_out, unsigned parts, silent_stream stream, const GrayKp* kp = nullptr) {
    const char* who = kFrameRgb8<FT> ? (kp ? "silent_gray_keypoints_u8x3" : "silent_gray_pass_u8x3") : kFrameBytes<FT> ? (kp ? "silent_gray_keypoints_u8" : "silent_gray_pass_u8") : kStoreHalf<ST> ? "silent_gray_pass_h" : "silent_gray_pass";
    if (!plan || !frames || !pyr || !cs_kernel) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (plan->ctx != ctx) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": plan belongs to another context");
    if constexpr (kFrameNarrow<FT>) {
        if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": uint8 frames are for single-channel plans");
        if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": uint8 frames with a SILENT_PLAN_ACCUM_F64 plan");
    }
    if constexpr (kStoreHalf<ST>) {
        if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": float16 storage is for single-channel plans");
        if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": float16 storage with a SILENT_PLAN_ACCUM_F64 plan");
    }
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": the plan must be single-channel");
    if (!cs_out && !end_out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": both outputs are NULL");
    if (end_out && !end_bank) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": end_bank is NULL");
    if (n_orient != 3 && n_orient != 4 && n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": n_orient must be 3, 4 or 8");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_frames must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    const PyrTab& pt = plan->tab;
    const int kopts = (int)ctx->tune[SILENT_TUNE_GRAY];  // A/B knob: bit4 disables the stream path (bit3, 32-row fused tiles, is ignored since round 6)
    const bool stream_path = plan->stream_ok && !(kopts & 16);
    // 1. non-unit levels of the pyramid: by the region kernel, unless the stream kernel of step 2 produces them
    //    from the same single read of the frame; plus the zero fill of canvases larger than their zoomed crop
    if (!(parts & 3u)) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": parts must name step 1 + 2 (bit 0) and / or step 3 (bit 1)");
    if (parts & 1u) {
        if constexpr (kFrameRgb8<FT>) TRY(launch_pyramid_u8x3(ctx, who, plan, frames, n_frames, pyr, s, false, !stream_path));
        else if constexpr (kFrameBytes<FT>) TRY(launch_pyramid_u8(ctx, who, plan, frames, n_frames, pyr, s, false, !stream_path));
        else TRY(launch_pyramid(ctx, who, plan, frames, n_frames, pyr, s, false, !stream_path));
    }
    // 2. unit levels: pyramid + CS + end in one kernel
    const int fth = kFusedTH;
    FusedTab64 ft;   // (the float32 kernels take its FusedTab part)
    std::memset(&ft, 0, sizeof(ft));
    bool is_unit[kMaxLevels] = {false};
    long long tiles = 0, unit_px = 0;
    GrayKp kpu{};   // the unit levels' plan level numbers travel with the keypoint epilogue's arguments
    if (kp) kpu = *kp;
    for (int l = 0; l < pt.n_levels; ++l) {
        const PyrLevelDev& d = pt.lv[l];
        if (d.kind != kPyrUnit) continue;
        is_unit[l] = true;
        if (kp) kpu.level[ft.n] = l;
        if (ft.n == 0)
            for (int j = 0; j < 6; ++j) {  // every unit level has the same taps ([1,26,66,26,1]/120 and the sixth, 2^-53)
                ft.wx[j] = plan->unit_w[j];
                ft.wy[j] = plan->unit_w[j];
                ft.w64[j] = plan->unit_w64[j];
            }
        FusedLevel& f = ft.lv[ft.n++];
        f.src_y0 = d.src_y0; f.src_x0 = d.src_x0; f.src_h = d.src_h; f.src_w = d.src_w;
        f.zoom_h = d.zoom_h; f.zoom_w = d.zoom_w; f.out_h = d.out_h; f.out_w = d.out_w;
        f.tiles_x = (d.out_w + kFusedTW - 1) / kFusedTW;
        f.tile_start = (int)tiles;
        f.px_off = pt.px_off[l];
        tiles += (long long)f.tiles_x * ((d.out_h + fth - 1) / fth);
        unit_px += (long long)d.out_h * d.out_w;
    }
    ft.tiles_per_frame = (int)tiles;
    ft.H = pt.H;
    ft.W = pt.W;
    ft.frame_px = pt.frame_px_out;
    const long long blocks = tiles * n_frames;
    if (blocks > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many tiles for one launch");
    if (blocks && (parts & 1u)) {
        GrayW w;
        std::memset(&w, 0, sizeof(w));
        std::memcpy(w.cs, cs_kernel, sizeof(float) * 9);
        if (end_bank) std::memcpy(w.end, end_bank, sizeof(float) * 9 * n_orient);
        ctx->prof_sample = ctx->profiling && (ctx->prof_calls++ % ctx->prof_period) == 0;
        const int prof_slot = ctx->prof_recorded % silent_ctx::kProfPairs;
        if (ctx->prof_sample) HIP_TRY(ctx, hipEventRecord(ctx->prof_ev[prof_slot][0], s));
        const GrayKp* kpp = kp ? &kpu : nullptr;
        if (stream_path) {
            const StreamTab& st = plan->stream;
            const unsigned sopts = (unsigned)((kopts >> 5) & 1);
#define STREAM_LAUNCH(K_, G_, L_)                                                                                  \
    if constexpr (kStoreHalf<ST>) launch_stream<K_, G_, L_, false, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, st, w, clip_hi, sopts, nullptr); \
    else if constexpr (kFrameNarrow<FT>) launch_stream<K_, G_, L_, false, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, st, w, clip_hi, sopts, kpp); \
    else if (plan->f64) launch_stream<K_, G_, L_, true, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, st, w, clip_hi, sopts, kpp); \
    else launch_stream<K_, G_, L_, false, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, st, w, clip_hi, sopts, kpp)
            if (plan->stream_layout == 1) {          // zoom ladders of ratio 1.4 .. e^.5: five rows of the first level in flight
                if (n_orient == 3) { STREAM_LAUNCH(3, 7, 1); }
                else if (n_orient == 4) { STREAM_LAUNCH(4, 7, 1); }
                else { STREAM_LAUNCH(8, 7, 1); }
            } else if (st.G <= 4) {
                if (n_orient == 3) { STREAM_LAUNCH(3, 4, 0); }
                else if (n_orient == 4) { STREAM_LAUNCH(4, 4, 0); }
                else { STREAM_LAUNCH(8, 4, 0); }
            } else {
                if (n_orient == 3) { STREAM_LAUNCH(3, 7, 0); }
                else if (n_orient == 4) { STREAM_LAUNCH(4, 7, 0); }
                else { STREAM_LAUNCH(8, 7, 0); }
            }
#undef STREAM_LAUNCH
        } else {
#define FUSED_LAUNCH(K_)                                                                                   \
    if constexpr (kStoreHalf<ST>) launch_fused<K_, false, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, w, clip_hi, nullptr); \
    else if constexpr (kFrameNarrow<FT>) launch_fused<K_, false, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, w, clip_hi, kpp); \
    else if (plan->f64) launch_fused<K_, true, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, w, clip_hi, kpp); \
    else launch_fused<K_, false, ST, FT>(blocks, s, frames, pyr, cs_out, end_out, ft, w, clip_hi, kpp)
            if (n_orient == 3) { FUSED_LAUNCH(3); }
            else if (n_orient == 4) { FUSED_LAUNCH(4); }
            else { FUSED_LAUNCH(8); }
#undef FUSED_LAUNCH
        }
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

// silent_gray_keypoints_dev (silent_peaks_api.hip): the whole pass with the keypoint epilogue in every kernel that writes `end`
int gray_pass_kp(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames, const float* cs_kernel,
                 const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out, float* end_out, const GrayKp& kp,
                 hipStream_t s) {
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, 3u,
                           (silent_stream)s, &kp);
}

int gray_pass_kp_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, const float* cs_kernel,
                    const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out, float* end_out, const GrayKp& kp,
                    hipStream_t s) {
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, 3u,
                           (silent_stream)s, &kp);
}

int gray_pass_kp_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const FrameRgb8* frames, int n_frames, const float* cs_kernel,
                      const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out, float* end_out, const GrayKp& kp,
                      hipStream_t s) {
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, 3u,
                           (silent_stream)s, &kp);
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
    if (!pyr) return fail(ctx, SILENT_E_INVALID, "silent_gray_line_end: NULL pointer");
    if (n_orient < 1 || n_orient > 8) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_line_end: n_orient must be 3, 4 or 8");
    long long px;
    TRY(check_levels(ctx, "silent_gray_line_end", levels, n_levels, n_frames, &px));
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
    if (!plan || !frames || !pyr) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass: NULL pointer");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass: n_frames must be >= 1");
    if (n_orient < 1 || n_orient > 8) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass: n_orient must be 3, 4 or 8");
    HostStage hs(ctx);
    const size_t b1 = (size_t)plan->tab.frame_px_out * n_frames * 4;
    const int x = hs.in(frames, (size_t)plan->tab.H * plan->tab.W * plan->tab.C * 4 * n_frames), p = hs.out(pyr, b1),
              cs = hs.out(cs_out, b1), end = hs.out(end_out, b1 * n_orient);
    return hs.run([&] {
        return silent_gray_pass_dev(ctx, plan, hs.dev<float>(x), n_frames, cs_kernel, end_bank, n_orient, clip_hi, hs.dev<float>(p),
                                    hs.dev<float>(cs), hs.dev<float>(end), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_gray_pass");
}

// ------------------------------------------------------------------------------------------ float16 storage of the CS and end maps
// The same pass, the two maps stored as IEEE binary16 (the ST = gray_half instantiations of the same kernels; silent_hip.h has the
// contract).  uint16_t in the C ABI: plain C has no half type.

SILENT_EXPORT int silent_gray_pass_h_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                                         const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                         uint16_t* cs_out, uint16_t* end_out, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr,
                           reinterpret_cast<gray_half*>(cs_out), reinterpret_cast<gray_half*>(end_out), parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_h_dev");
}

SILENT_EXPORT int silent_gray_pass_h(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                                     const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                     uint16_t* cs_out, uint16_t* end_out) try {
    NEED_CTX(ctx);
    if (!plan || !frames || !pyr) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass_h: NULL pointer");
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_h: float16 storage is for single-channel plans");
    if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_h: float16 storage with a SILENT_PLAN_ACCUM_F64 plan");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass_h: n_frames must be >= 1");
    if (n_orient != 3 && n_orient != 4 && n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_h: n_orient must be 3, 4 or 8");
    HostStage hs(ctx);
    const size_t px = (size_t)plan->tab.frame_px_out * n_frames;
    const int x = hs.in(frames, (size_t)plan->tab.H * plan->tab.W * 4 * n_frames), p = hs.out(pyr, px * 4), cs = hs.out(cs_out, px * 2),
              end = hs.out(end_out, px * 2 * n_orient);
    return hs.run([&] {
        return silent_gray_pass_h_dev(ctx, plan, hs.dev<float>(x), n_frames, cs_kernel, end_bank, n_orient, clip_hi, hs.dev<float>(p),
                                      hs.dev<uint16_t>(cs), hs.dev<uint16_t>(end), 3u, nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_h");
}

// ------------------------------------------------------------------------------------------ uint8 frames
// The same pass reading uint8 frames as they are (the FT = unsigned char instantiations of the frame-reading kernels; silent_hip.h
// has the contract): the byte is widened in a register at the load, so every output is the float32-frame entry point's, bit for bit.

SILENT_EXPORT int silent_gray_pass_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                          const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                          void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    if (maps_f16)
        return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr,
                               static_cast<gray_half*>(cs_out), static_cast<gray_half*>(end_out), parts, stream);
    return gray_pass_parts(ctx, plan, frames, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, static_cast<float*>(cs_out),
                           static_cast<float*>(end_out), parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8_dev");
}

SILENT_EXPORT int silent_gray_pass_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                      const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                      void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    if (!plan || !frames || !pyr) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass_u8: NULL pointer");
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_u8: uint8 frames are for single-channel plans");
    if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_u8: uint8 frames with a SILENT_PLAN_ACCUM_F64 plan");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass_u8: n_frames must be >= 1");
    if (n_orient != 3 && n_orient != 4 && n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_u8: n_orient must be 3, 4 or 8");
    HostStage hs(ctx);
    const size_t px = (size_t)plan->tab.frame_px_out * n_frames, eb = maps_f16 ? 2 : 4;
    // (the frames are bytes: H * W * n of them, not * 4)
    const int x = hs.in(frames, (size_t)plan->tab.H * plan->tab.W * n_frames), p = hs.out(pyr, px * 4), cs = hs.out(cs_out, px * eb),
              end = hs.out(end_out, px * eb * n_orient);
    return hs.run([&] {
        return silent_gray_pass_u8_dev(ctx, plan, hs.dev<uint8_t>(x), n_frames, cs_kernel, end_bank, n_orient, clip_hi, hs.dev<float>(p),
                                       hs.dev<char>(cs), hs.dev<char>(end), maps_f16, 3u, nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8");
}

// ------------------------------------------------------------------------------------------ interleaved 3-channel uint8 frames
// The same pass reading [n, H, W, 3] uint8 colour frames as they are (the FT = FrameRgb8 instantiations of the frame-reading kernels;
// silent_hip.h has the contract): each pixel's value (b0 + b1 + b2) * float32(1/3) is formed in registers at the load, so every output
// is the float32-frame entry point's on the frame of values, bit for bit.  The plan is single-channel: the layout belongs to the call.

SILENT_EXPORT int silent_gray_pass_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                            const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                            void* cs_out, void* end_out, int maps_f16, unsigned parts, silent_stream stream) try {
    NEED_CTX(ctx);
    const FrameRgb8* px = reinterpret_cast<const FrameRgb8*>(frames);
    if (maps_f16)
        return gray_pass_parts(ctx, plan, px, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr,
                               static_cast<gray_half*>(cs_out), static_cast<gray_half*>(end_out), parts, stream);
    return gray_pass_parts(ctx, plan, px, n_frames, cs_kernel, end_bank, n_orient, clip_hi, pyr, static_cast<float*>(cs_out),
                           static_cast<float*>(end_out), parts, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8x3_dev");
}

SILENT_EXPORT int silent_gray_pass_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                        const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, float* pyr,
                                        void* cs_out, void* end_out, int maps_f16) try {
    NEED_CTX(ctx);
    if (!plan || !frames || !pyr) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass_u8x3: NULL pointer");
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_u8x3: uint8 frames are for single-channel plans");
    if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_u8x3: uint8 frames with a SILENT_PLAN_ACCUM_F64 plan");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, "silent_gray_pass_u8x3: n_frames must be >= 1");
    if (n_orient != 3 && n_orient != 4 && n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, "silent_gray_pass_u8x3: n_orient must be 3, 4 or 8");
    HostStage hs(ctx);
    const size_t px = (size_t)plan->tab.frame_px_out * n_frames, eb = maps_f16 ? 2 : 4;
    // (the frames are interleaved colour bytes: 3 * H * W * n of them)
    const int x = hs.in(frames, (size_t)3 * plan->tab.H * plan->tab.W * n_frames), p = hs.out(pyr, px * 4), cs = hs.out(cs_out, px * eb),
              end = hs.out(end_out, px * eb * n_orient);
    return hs.run([&] {
        return silent_gray_pass_u8x3_dev(ctx, plan, hs.dev<uint8_t>(x), n_frames, cs_kernel, end_bank, n_orient, clip_hi, hs.dev<float>(p),
                                         hs.dev<char>(cs), hs.dev<char>(end), maps_f16, 3u, nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_gray_pass_u8x3");
}
