// The grayscale pass from the frame (silent_gray_api.hip, silent_gray16_api.hip): the bodies the entry points of every frame kind share
// -- checks, the launches of the pass, the map storage, the host-pointer form.  Templates on the frame kind FT (and the map storage ST),
// instantiated by the unit that defines a frame kind's entry points: float and the uint8 kinds in silent_gray_api.hip, the uint16 kinds
// in silent_gray16_api.hip (a unit of their own: the units compile side by side, and silent_gray_api is the slowest of them).
#pragma once

#include "silent_plan.h"

using namespace silent;

// CS + end on the levels of a packed pyramid (gray_line_end_kernel; defined, and instantiated for the two map storages, in
// silent_gray_api.hip).  skip: levels to leave out; kp: the keypoint epilogue; f64: the F64 kernel (F64 plans only)
template <typename ST>
int launch_gray(silent_ctx* ctx, const char* who, const float* pyr, const silent_extent* levels, int n_levels, int n_frames,
                const float* cs_kernel, const float* end_bank, int n_orient, float clip_hi, ST* cs_out, ST* end_out, hipStream_t s,
                const bool* skip, const GrayKp* kp = nullptr, bool f64 = false);
extern template int launch_gray<float>(silent_ctx*, const char*, const float*, const silent_extent*, int, int, const float*, const float*, int, float,
                                       float*, float*, hipStream_t, const bool*, const GrayKp*, bool);
extern template int launch_gray<gray_half>(silent_ctx*, const char*, const float*, const silent_extent*, int, int, const float*, const float*, int,
                                           float, gray_half*, gray_half*, hipStream_t, const bool*, const GrayKp*, bool);

// everything silent_gray_pass*_dev refuses, before a launch (and, in the host forms, before the batch is staged); FT: the frame kind of
// the ENTRY POINT (the view entry points check as a strided kind whatever kind then reads the view), has_frames: its frames are not NULL
template <typename FT>
static int gray_pass_checks(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, bool has_frames, int n_frames,
                            const float* cs_kernel, const float* end_bank, int n_orient, const float* pyr, const void* cs_out,
                            const void* end_out, bool f16, unsigned parts) {
    if (!plan || !has_frames || !pyr || !cs_kernel) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (plan->ctx != ctx) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": plan belongs to another context");
    if constexpr (kFrameNarrow<FT>) TRY(check_narrow_frames<FT>(ctx, who, plan));
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
