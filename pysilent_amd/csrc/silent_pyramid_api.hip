// libsilent_hip.so -- the zoom pyramid (silent_pyramid.h, silent_walk_rgb.h, pyramid_stream_kernel of silent_gray.h): plans (float64 tap tables,
// scipy-identical; row programs and column records of the single-read kernels: built by silent_plan_build.h, uploaded here) and their launches.
#include "silent_plan_build.h"

#include <memory>

using namespace silent;

// ------------------------------------------------------------------------------------------ pyramid plan
// ONE device allocation for host blobs: every part starts on a 256-byte boundary (pad_last: the last one is padded too), one hipMemcpy
// per part, off[i] its offset.  On a failure nothing stays allocated, *dev is NULL and *step (if given) names the call that failed.
typedef std::pair<const void*, size_t> HostPart;   // (pointer, bytes)
static hipError_t upload(void** dev, const std::vector<HostPart>& parts, size_t* off, bool pad_last = true, const char** step = nullptr) {
    size_t total = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        off[i] = total;
        total += i + 1 < parts.size() || pad_last ? align_up(parts[i].second) : parts[i].second;
    }
    const char* at = "hipMalloc";
    hipError_t e = hipMalloc(dev, total);
    if (e != hipSuccess) *dev = nullptr;
    for (size_t i = 0; i < parts.size() && e == hipSuccess; ++i) {
        at = "hipMemcpy";
        e = hipMemcpy((char*)*dev + off[i], parts[i].first, parts[i].second, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (*dev) (void)hipFree(*dev);
        *dev = nullptr;
        if (step) *step = at;
    }
    return e;
}

SILENT_EXPORT int silent_pyramid_plan_create_ex(silent_ctx* ctx, int frame_h, int frame_w, int channels,
                                                const silent_pyr_level* levels, int n_levels, unsigned flags,
                                                silent_pyramid_plan** out) try {
    NEED_CTX(ctx);
    const char* who = "silent_pyramid_plan_create";
    // ---- validate
    if (!out || !levels) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    *out = nullptr;
    if (flags & ~SILENT_PLAN_ACCUM_F64) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": unknown flag bits");
    if (frame_h < 1 || frame_w < 1 || (long long)frame_h * frame_w > (1ll << 30))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": bad frame extent");
    if (channels != 1 && channels != 3)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": channels must be 1 or 3");
    const bool f64 = (flags & SILENT_PLAN_ACCUM_F64) != 0;
    if (f64 && channels != 1)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": float64 accumulation needs a single-channel plan");
    if (n_levels < 1 || n_levels > kMaxLevels)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_levels must be in [1, " + std::to_string(kMaxLevels) + "]");
    // (the plan frees its tables itself: every exit below, an exception included, is a plain return)
    std::unique_ptr<silent_pyramid_plan> plan(new (std::nothrow) silent_pyramid_plan());
    if (!plan) return fail(ctx, SILENT_E_NOMEM, std::string(who) + ": out of host memory");
    plan->ctx = ctx;
    plan->flags = flags;
    plan->f64 = f64;
    PyrTab& tab = plan->tab;
    const int bad = build_levels(tab, frame_h, frame_w, channels, levels, n_levels, plan->extents);
    if (bad >= 0) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": level " + std::to_string(bad) + " geometry is invalid");
    // ---- tap and region tables
    AxisTables ax;
    if (!build_axis_tables(tab, f64, ax, plan->unit_w, plan->unit_w64))
        return fail(ctx, SILENT_E_HIP, std::string(who) + ": internal error: a tap fell outside its staged region");
    size_t off[6];            // (offsets of the parts of an upload)
    const char* step = "";
    hipError_t e = upload(&plan->tables, {{ax.xidx.data(), ax.xidx.size() * 4}, {ax.xw.data(), ax.xw.size() * 4}, {ax.yidx.data(), ax.yidx.size() * 4},
                                          {ax.yw.data(), ax.yw.size() * 4}, {ax.xreg.data(), ax.xreg.size() * 4}, {ax.yreg.data(), ax.yreg.size() * 4}},
                          off, true, &step);
    if (e != hipSuccess)
        return fail(ctx, std::strcmp(step, "hipMalloc") ? SILENT_E_HIP : SILENT_E_NOMEM, std::string(who) + ": " + step + ": " + hipGetErrorString(e));
    const char* t = (const char*)plan->tables;
    tab.xidx = (const int*)(t + off[0]); tab.xw = (const float*)(t + off[1]);
    tab.yidx = (const int*)(t + off[2]); tab.yw = (const float*)(t + off[3]);
    tab.xreg = (const int*)(t + off[4]); tab.yreg = (const int*)(t + off[5]);
    if (f64) {
        e = upload(&plan->tables64, {{ax.xw64.data(), ax.xw64.size() * 8}, {ax.yw64.data(), ax.yw64.size() * 8}}, off);
        if (e != hipSuccess) return fail(ctx, SILENT_E_NOMEM, std::string(who) + ": float64 tap tables: " + hipGetErrorString(e));
        static_cast<PyrTab&>(plan->tab64) = tab;
        plan->tab64.xw64 = (const double*)plan->tables64;
        plan->tab64.yw64 = (const double*)((char*)plan->tables64 + off[1]);
    }
    const int classic = same_crop_unit(tab);
    // ---- single-read stream path (see gray_stream_kernel): a classic single-channel plan, in the first slot layout that holds it.  (A
    // failed upload here or for the walk is silent: the plan stays on the other kernels.)
    for (int layout = 0; layout < 2 && channels == 1 && classic >= 0 && !plan->stream_ok; ++layout) {
        StreamTables st;
        if (!build_stream_tables(tab, ax, classic, layout, f64, st, plan->stream)) continue;
        if (upload(&plan->stream_tables, {{st.prog.data(), st.prog.size() * 4}, {st.hdr.data(), st.hdr.size() * 4}, {st.rec.data(), st.rec.size() * 4}}, off) != hipSuccess)
            continue;
        const char* s = (const char*)plan->stream_tables;
        plan->stream.row_prog = (const int*)(s + off[0]);
        plan->stream.col_hdr = (const int*)(s + off[1]);
        plan->stream.col_rec = (const int*)(s + off[2]);
        plan->stream_unit_level = classic;
        plan->stream_layout = layout;
        plan->stream_ok = true;
    }
    // ---- walk plans of pyramid_walk3_kernel (3 channels): the first candidate, at the widest wave tile, whose tables can be built
    if (channels == 3)
        for (const WalkCandidate& hp : walk_candidates(tab, ctx->tune[SILENT_TUNE_PYRAMID]))
            for (int px : {36, 32, 28, 24}) {
                if (plan->walk_pyr_ok) break;                     // (built: every later candidate ends here at once)
                WalkTables wt;
                if (!build_walk_tables(tab, ax, hp, px, plan->unit_w, wt)) continue;
                if (upload(&plan->walk_tables, {{wt.blob.data(), wt.blob.size() * 4}}, off, false) != hipSuccess) break;   // (the next candidate)
                const int* base = (const int*)plan->walk_tables;
                for (size_t pi = 0; pi < hp.size(); ++pi) {
                    wt.args.plan[pi].pyr.row_prog = base + wt.offs[3 * pi];
                    wt.args.plan[pi].pyr.col_hdr = base + wt.offs[3 * pi + 1];
                    wt.args.plan[pi].pyr.col_rec = base + wt.offs[3 * pi + 2];
                }
                plan->walk = wt.args;
                plan->walk_border = wt.border;
                plan->walk_px = px;
                plan->walk_G = wt.Gp;
                plan->walk_pyr_ok = true;
            }
    *out = plan.release();
    return SILENT_OK;
} catch (...) {
    return on_exception(ctx, "silent_pyramid_plan_create");
}

SILENT_EXPORT int silent_pyramid_plan_create(silent_ctx* ctx, int frame_h, int frame_w, int channels,
                                             const silent_pyr_level* levels, int n_levels,
                                             silent_pyramid_plan** out) {
    return silent_pyramid_plan_create_ex(ctx, frame_h, frame_w, channels, levels, n_levels, 0u, out);
}

SILENT_EXPORT int silent_pyramid_plan_flags(const silent_pyramid_plan* plan, unsigned* flags) try {
    if (!plan || !flags) return SILENT_E_INVALID;
    *flags = plan->flags;
    return SILENT_OK;
} catch (...) {
    return on_exception(nullptr, "silent_pyramid_plan_flags");
}

SILENT_EXPORT void silent_pyramid_plan_destroy(silent_pyramid_plan* plan) try {
    delete plan;
} catch (...) {
}

template <int G, int PX, typename FT>
static int walk3_blocks_per_cu() {
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pyramid_walk3_kernel<G, PX, FT>, kW3Threads, 0);
    (void)hipGetLastError();
    return std::max(per_cu, 1);
}

// Per-launch decomposition of the plan's walks (any batch size): strips of 4 x PX pixels, cut into segments of ONE height for
// every plan of the launch -- the height that makes about 3.5 blocks per block the chip holds (but not below 32 rows: every
// segment walks 8 rows of halo).  Rounds 2 - 4 minimised ceil(blocks / resident blocks) x (segment rows + 8) per plan; that
// model is right for one plan of equal blocks that fills the chip a few times (config 3: 4 ... 20 segments per frame measured
// flat within 3 %, both rules land there) and wrong for the reference layout, where it gave the union plan exactly one round of
// 224-row blocks beside the unit plan's short ones: 0.199 ms, against 0.165 ms with 12 - 20 segments (profiles/r05_experiments.txt 7).
// FT: the frame kind of the launch (the occupancy asked about is that of the instantiation that is launched).
template <typename FT>
static bool walk3_plan(const silent_ctx* ctx, const silent_pyramid_plan* plan, int n_frames, Walk3Args* wa) {
    if (plan->tab.C != 3 || !plan->walk_pyr_ok) return false;
    *wa = plan->walk;
    const int px = plan->walk_px;
    int per_cu = 1;
#define PER_CU(PX_) case PX_: per_cu = plan->walk_G <= 4 ? walk3_blocks_per_cu<4, PX_, FT>() : walk3_blocks_per_cu<7, PX_, FT>(); break
    switch (px) { PER_CU(36); PER_CU(32); PER_CU(28); PER_CU(24); default: return false; }
#undef PER_CU
    const long long resident = (long long)per_cu * ctx->n_cus;
    long long strip_rows = 0;                                   // rows x strips of every plan, one frame
    for (int pi = 0; pi < wa->n_plans; ++pi) {
        Walk3Plan& w = wa->plan[pi];
        w.strips_x = (w.out_w + kW3NC * px - 1) / (kW3NC * px);
        strip_rows += (long long)w.strips_x * w.out_h;
    }
    // (round 6: a launch that stays within a quarter of the chip even in 8-row segments -- a single camera frame -- is pure latency,
    // one block's walk of segment rows + 8: 8-row segments there, profiles/r06_experiments.txt 8)
    const long long min_rows = (strip_rows * n_frames + 7) / 8 * 4 <= resident ? 8 : 32;
    const long long target = std::max<long long>(min_rows, (2 * strip_rows * n_frames + 7 * resident - 1) / (7 * resident));   // rows per segment
    long long block0 = 0;
    for (int pi = 0; pi < wa->n_plans; ++pi) {
        Walk3Plan& w = wa->plan[pi];
        const int segs = (int)std::max<long long>(1, (w.out_h + target / 2) / target);
        int seg_rows = (w.out_h + segs - 1) / segs;
        seg_rows = (seg_rows + kWalkCH - 1) / kWalkCH * kWalkCH;
        w.seg_rows = seg_rows;
        w.segs_y = (w.out_h + seg_rows - 1) / seg_rows;
        w.block0 = (int)block0;
        block0 += (long long)w.strips_x * w.segs_y;
    }
    if (block0 * n_frames > 0x7fffffffll) return false;
    wa->blocks_per_frame = (int)block0;
    return true;
}

// everything silent_pyramid*_dev refuses, before a launch (and, in the host forms, before the batch is staged); FT: the frame kind of
// the ENTRY POINT (the view entry points check as a strided kind whatever kind then reads the view), has_frames: its frames are not NULL
template <typename FT>
static int pyramid_checks(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, bool has_frames, int n_frames, const float* pyr) {
    if (!plan || !has_frames || !pyr) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (plan->ctx != ctx) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": plan belongs to another context");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_frames must be >= 1");
    if constexpr (kFrameNarrow<FT>) TRY(check_narrow_frames<FT>(ctx, who, plan));
    return SILENT_OK;
}

// The launches of a 3-channel plan on frame kind FT -- float, unsigned char (packed interleaved uint8 colour frames,
// silent_pyramid_rgb8) or ViewRgb (the same bytes in a strided view, silent_pyramid_rgb8_view; `frames` points to the host struct):
// ONE body, so every kind takes the same route on the same plan under the same PYRAMID knob bits.
template <typename FT>
static int launch_pyramid3(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const FT* frames, int n_frames, float* pyr,
                           hipStream_t s, bool with_unit, bool with_region, long long b_unit, long long b_region) {
    const PyrTab& tab = plan->tab;
    const unsigned kopts = ctx->tune[SILENT_TUNE_PYRAMID];
    Walk3Args w3t;
    if (plan->walk_pyr_ok && with_unit && with_region && !(kopts & 3u) && walk3_plan<FT>(ctx, plan, n_frames, &w3t)) {
        // single-read RGB pyramid (pyramid_walk3_kernel, silent_walk_rgb.h); PYRAMID knob bits 1 / 2: unit + region kernels
        // union plans: the inner levels' first / last output rows and columns -- the last blocks of the same launch (PYRAMID knob 8:
        // a launch of their own behind the walk)
        const long long bthreads = (long long)plan->walk_border.per_frame * 3 * n_frames;
        const long long bblocks = (bthreads + 255) / 256;
        const bool border_inside = bblocks > 0 && !(kopts & 8u);
        const long long wblocks = (long long)n_frames * w3t.blocks_per_frame + (border_inside ? bblocks : 0);
        if (wblocks > 0x7fffffffll || bblocks > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many blocks for one launch");
        WalkBorderArgs wb;
        std::memset(&wb, 0, sizeof(wb));
        wb.first = 0x7fffffff;
        if (border_inside) {
            wb.first = (int)((long long)n_frames * w3t.blocks_per_frame);
            wb.n_frames = n_frames;
            wb.tab = tab;
            wb.bt = plan->walk_border;
        }
#define WALK3(G_, PX_) hipLaunchKernelGGL((pyramid_walk3_kernel<G_, PX_, FT>), dim3((unsigned)wblocks), dim3(kW3Threads), 0, s, kernel_frames(frames), pyr, w3t, wb)
#define WALK3_PX(PX_) case PX_: if (plan->walk_G <= 4) WALK3(4, PX_); else WALK3(7, PX_); break
        switch (plan->walk_px) { WALK3_PX(36); WALK3_PX(32); WALK3_PX(28); WALK3_PX(24); default: break; }   // (walk3_plan refuses any other)
#undef WALK3_PX
#undef WALK3
        if (bblocks > 0 && !border_inside)
            hipLaunchKernelGGL((pyramid_border_kernel<3, FT>), dim3((unsigned)bblocks), dim3(256), 0, s, kernel_frames(frames), pyr, tab, plan->walk_border, n_frames);
        return SILENT_OK;
    }
    if (b_unit) hipLaunchKernelGGL((pyramid_unit_kernel<3, false, FT>), dim3((unsigned)b_unit), dim3(256), 0, s, kernel_frames(frames), pyr, tab);
    if (b_region) hipLaunchKernelGGL((pyramid_region_kernel<3, false, FT>), dim3((unsigned)b_region), dim3(256), 0, s, kernel_frames(frames), pyr, tab);
    return SILENT_OK;
}

template <typename FT>
int launch_pyramid(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const FT* frames, int n_frames, float* pyr,
                   hipStream_t s, bool with_unit, bool with_region) {
    TRY(pyramid_checks<FT>(ctx, who, plan, frames != nullptr, n_frames, pyr));
    const PyrTab& tab = plan->tab;
    const long long b_unit = with_unit ? (long long)tab.unit_tiles_per_frame * n_frames : 0;
    const long long b_region = (with_region && tab.n_general) ? (long long)tab.regions_x * tab.regions_y * n_frames : 0;
    const long long b_zero = (long long)tab.zero_chunks_per_frame * n_frames;
    if (b_unit > 0x7fffffffll || b_region > 0x7fffffffll || b_zero > 0x7fffffffll)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many tiles for one launch");
    const unsigned kopts = ctx->tune[SILENT_TUNE_PYRAMID];  // 1: no stream kernel
    if (plan->stream_ok && with_unit && with_region && !(kopts & 1u)) {
        // single-read pyramid: frame -> every level in one kernel (pyramid_stream_kernel; single-channel plans only:
        // on interleaved RGB the stride-3 accesses of the same kernel made it 1.5x SLOWER than unit + region kernels)
        FusedTab64 ft = fused_tab(plan);
        fused_add_level(ft, tab, plan->stream_unit_level);
        const long long blocks = (long long)ft.tiles_per_frame * n_frames;
        if (blocks > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many tiles for one launch");
        with_gray_mode<float, FT>(false, plan->f64, [&](auto, auto F64) {
            const FusedTabT<decltype(F64)::value>& t = ft;   // (the float32 kernels take its FusedTab part)
            with_stream_layout(plan, [&](auto G, auto L) {
                hipLaunchKernelGGL((pyramid_stream_kernel<1, decltype(G)::value, decltype(L)::value, decltype(F64)::value, FT>),
                                   dim3((unsigned)blocks), dim3(64 * kFusedWaves), 0, s, kernel_frames(frames), pyr, t, plan->stream);
            });
        });
    } else if constexpr (kFrameNarrow<FT>) {   // (single-channel, float32 accumulation: checked above)
        if (b_unit) hipLaunchKernelGGL((pyramid_unit_kernel<1, false, FT>), dim3((unsigned)b_unit), dim3(256), 0, s, kernel_frames(frames), pyr, tab);
        if (b_region)
            hipLaunchKernelGGL((pyramid_region_kernel<1, false, FT>), dim3((unsigned)b_region), dim3(256), 0, s, kernel_frames(frames), pyr, tab);
    } else if (tab.C == 3) {
        TRY(launch_pyramid3(ctx, who, plan, frames, n_frames, pyr, s, with_unit, with_region, b_unit, b_region));
    } else if (plan->f64) {   // (single-channel)
        if (b_unit) hipLaunchKernelGGL((pyramid_unit_kernel<1, true>), dim3((unsigned)b_unit), dim3(256), 0, s, frames, pyr, plan->tab64);
        if (b_region) hipLaunchKernelGGL((pyramid_region_kernel<1, true>), dim3((unsigned)b_region), dim3(256), 0, s, frames, pyr, plan->tab64);
    } else {
        if (b_unit) hipLaunchKernelGGL(pyramid_unit_kernel<1>, dim3((unsigned)b_unit), dim3(256), 0, s, frames, pyr, tab);
        if (b_region) hipLaunchKernelGGL(pyramid_region_kernel<1>, dim3((unsigned)b_region), dim3(256), 0, s, frames, pyr, tab);
    }
    if (b_zero && tab.C == 1) hipLaunchKernelGGL(pyramid_zero_kernel<1>, dim3((unsigned)b_zero), dim3(256), 0, s, pyr, tab);
    else if (b_zero) hipLaunchKernelGGL(pyramid_zero_kernel<3>, dim3((unsigned)b_zero), dim3(256), 0, s, pyr, tab);
    return check_launch(ctx, who);
}

#define X(FT) \
    template int launch_pyramid<FT>(silent_ctx*, const char*, const silent_pyramid_plan*, const FT*, int, float*, hipStream_t, bool, bool);
SILENT_FRAME_TYPES(X)
#undef X

SILENT_EXPORT int silent_pyramid_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames,
                                     int n_frames, float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return launch_pyramid(ctx, "silent_pyramid", plan, frames, n_frames, pyr, (hipStream_t)stream, true);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_dev");
}

// ------------------------------------------------------------------------------------------ whole gray pass

SILENT_EXPORT int silent_pyramid_plan_is_streamable(const silent_pyramid_plan* plan) try {
    return plan && plan->stream_ok ? 1 : 0;
} catch (...) {
    return on_exception(nullptr, "silent_pyramid_plan_is_streamable");
}

SILENT_EXPORT int silent_pyramid_plan_walk_plans(const silent_pyramid_plan* plan, int* pixels_per_wave) try {
    if (pixels_per_wave) *pixels_per_wave = plan && plan->walk_pyr_ok ? plan->walk_px : 0;
    return plan && plan->walk_pyr_ok ? plan->walk.n_plans : 0;
} catch (...) {
    return on_exception(nullptr, "silent_pyramid_plan_walk_plans");
}

// The host-pointer forms and the uint8 frame kinds (silent_hip.h has the contracts: the pyramid of uint8 frames is the float32-frame
// call's bit for bit -- a byte is widened at the load, an interleaved colour pixel becomes (b0 + b1 + b2) * float32(1/3) there;
// single-channel plans without SILENT_PLAN_ACCUM_F64: the plan describes the pyramid, the frame layout belongs to the call).
template <typename FT>
static int pyramid_host(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, float* pyr) {
    const char* who = entry_name<FT>(kPyramid);
    TRY(pyramid_checks<FT>(ctx, who, plan, frames != nullptr, n_frames, pyr));
    HostStage hs(ctx);
    const int x = hs.in(frames_host(frames), frames_bytes(plan, frames, n_frames)),
              o = hs.out(pyr, (size_t)plan->tab.frame_px_out * plan->tab.C * 4 * n_frames);
    return hs.run([&] {
        const StagedFrames<FT> staged(frames, hs.dev<char>(x));
        return launch_pyramid(ctx, who, plan, staged.p, n_frames, hs.dev<float>(o), nullptr, true);
    });
}

// Strided uint8 views (silent_hip.h): the view's own refusals and those of the *_u8 form under the view's name, then the frame kind
// that reads it (with_view: a packed view takes the packed kernels).
static int pyramid_view(silent_ctx* ctx, const char* who, bool host, const silent_pyramid_plan* plan, const silent_frame_view* view, int n_frames,
                        float* pyr, silent_stream stream) {
    TRY(check_view(ctx, who, plan, view, n_frames, nullptr));
    TRY(pyramid_checks<View8>(ctx, who, plan, true, n_frames, pyr));
    return with_view(plan, view, n_frames, [&](auto frames) {
        if (host) return pyramid_host(ctx, plan, frames, n_frames, pyr);
        return launch_pyramid(ctx, who, plan, frames, n_frames, pyr, (hipStream_t)stream, true);
    });
}

SILENT_EXPORT int silent_pyramid_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                          float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_view(ctx, "silent_pyramid_view", false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_view_dev");
}

SILENT_EXPORT int silent_pyramid_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                      float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_view(ctx, "silent_pyramid_view", true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_view");
}

SILENT_EXPORT int silent_pyramid(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames,
                                 float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_host(ctx, plan, frames, n_frames, pyr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid");
}

SILENT_EXPORT int silent_pyramid_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                        float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return launch_pyramid(ctx, "silent_pyramid_u8", plan, frames, n_frames, pyr, (hipStream_t)stream, true);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_u8_dev");
}

SILENT_EXPORT int silent_pyramid_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                    float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_host(ctx, plan, frames, n_frames, pyr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_u8");
}

SILENT_EXPORT int silent_pyramid_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                          float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return launch_pyramid(ctx, "silent_pyramid_u8x3", plan, rgb8(frames), n_frames, pyr, (hipStream_t)stream, true);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_u8x3_dev");
}

SILENT_EXPORT int silent_pyramid_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                      float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_host(ctx, plan, rgb8(frames), n_frames, pyr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_u8x3");
}

// uint16 frames (silent_hip.h): the *_u8 forms with an unsigned 16-bit element, 2-byte aligned; a strided uint16 view with the view's own
// refusals first (check_view16), then the frame kind that reads it (with_view16: a packed view takes the packed kernels).
SILENT_EXPORT int silent_pyramid_u16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                                         float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    TRY(check_u16_aligned(ctx, "silent_pyramid_u16", frames));
    return launch_pyramid(ctx, "silent_pyramid_u16", plan, frames, n_frames, pyr, (hipStream_t)stream, true);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_u16_dev");
}

SILENT_EXPORT int silent_pyramid_u16(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames,
                                     float* pyr) try {
    NEED_CTX(ctx);
    TRY(check_u16_aligned(ctx, "silent_pyramid_u16", frames));
    return pyramid_host(ctx, plan, frames, n_frames, pyr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_u16");
}

static int pyramid_view16(silent_ctx* ctx, const char* who, bool host, const silent_pyramid_plan* plan, const silent_frame_view16* view,
                          int n_frames, float* pyr, silent_stream stream) {
    TRY(check_view16(ctx, who, plan, view, n_frames, nullptr));
    TRY(pyramid_checks<View16>(ctx, who, plan, true, n_frames, pyr));
    return with_view16(plan, view, n_frames, [&](auto frames) {
        if (host) return pyramid_host(ctx, plan, frames, n_frames, pyr);
        return launch_pyramid(ctx, who, plan, frames, n_frames, pyr, (hipStream_t)stream, true);
    });
}

SILENT_EXPORT int silent_pyramid_view16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                            float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_view16(ctx, "silent_pyramid_view16", false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_view16_dev");
}

SILENT_EXPORT int silent_pyramid_view16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                        float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_view16(ctx, "silent_pyramid_view16", true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_view16");
}

// Packed interleaved uint8 colour frames for 3-channel plans (silent_hip.h): byte c of pixel (y, x) enters as (float)byte at the load,
// so the pyramid is the float32-frame call's on the widened frames bit for bit, on the route launch_pyramid takes for float frames.
// (single: the entry point a single-channel plan is pointed to)
static int pyramid_rgb8_checks(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, bool has_frames, int n_frames,
                               const float* pyr, const char* single = "silent_pyramid_u8x3") {
    TRY(pyramid_checks<float>(ctx, who, plan, has_frames, n_frames, pyr));
    if (plan->tab.C != 3)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": interleaved uint8 colour frames are for 3-channel plans (a single-channel plan takes them through " + single + ")");
    return SILENT_OK;
}

// FT: unsigned char, ViewRgb (silent_pyramid_rgb8_view on a view that is not packed), Nv12 (silent_pyramid_nv12), P010
// (silent_pyramid_p010), Yuv (silent_pyramid_yuv) or Yuv16 (silent_pyramid_yuv16); all but the first are checked by the caller
template <typename FT>
static int launch_pyramid_rgb8(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const FT* frames, int n_frames,
                               float* pyr, hipStream_t s) {
    if constexpr (!silent::kFrameRgbSrc<FT>) TRY(pyramid_rgb8_checks(ctx, who, plan, frames != nullptr, n_frames, pyr));
    const PyrTab& tab = plan->tab;
    const long long b_unit = (long long)tab.unit_tiles_per_frame * n_frames;
    const long long b_region = tab.n_general ? (long long)tab.regions_x * tab.regions_y * n_frames : 0;
    const long long b_zero = (long long)tab.zero_chunks_per_frame * n_frames;
    if (b_unit > 0x7fffffffll || b_region > 0x7fffffffll || b_zero > 0x7fffffffll)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many tiles for one launch");
    TRY(launch_pyramid3<FT>(ctx, who, plan, frames, n_frames, pyr, s, true, true, b_unit, b_region));
    if (b_zero) hipLaunchKernelGGL(pyramid_zero_kernel<3>, dim3((unsigned)b_zero), dim3(256), 0, s, pyr, tab);
    return check_launch(ctx, who);
}

SILENT_EXPORT int silent_pyramid_rgb8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                          float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return launch_pyramid_rgb8(ctx, "silent_pyramid_rgb8", plan, frames, n_frames, pyr, (hipStream_t)stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_rgb8_dev");
}

SILENT_EXPORT int silent_pyramid_rgb8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames,
                                      float* pyr) try {
    NEED_CTX(ctx);
    const char* who = "silent_pyramid_rgb8";
    TRY(pyramid_rgb8_checks(ctx, who, plan, frames != nullptr, n_frames, pyr));
    HostStage hs(ctx);
    const int x = hs.in(frames, (size_t)plan->tab.H * plan->tab.W * 3 * n_frames),
              o = hs.out(pyr, (size_t)plan->tab.frame_px_out * 3 * 4 * n_frames);
    return hs.run([&] { return launch_pyramid_rgb8(ctx, who, plan, hs.dev<uint8_t>(x), n_frames, hs.dev<float>(o), nullptr); });
} catch (...) {
    return on_exception(ctx, "silent_pyramid_rgb8");
}

// The same pixels in a strided view (silent_hip.h): the view's own refusals, then those of silent_pyramid_rgb8, both under this name;
// a packed view takes the packed kernels (with_rgb_view).  The host form stages the view's span, not a byte more.
static int pyramid_rgb8_view(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const silent_frame_view* view, int n_frames, float* pyr,
                             silent_stream stream) {
    const char* who = "silent_pyramid_rgb8_view";
    size_t span = 0;
    TRY(check_rgb_view(ctx, who, plan, view, n_frames, &span));
    TRY(pyramid_rgb8_checks(ctx, who, plan, true, n_frames, pyr, "silent_pyramid_view"));
    if (!host)
        return with_rgb_view(plan, view, n_frames, [&](auto frames) { return launch_pyramid_rgb8(ctx, who, plan, frames, n_frames, pyr, (hipStream_t)stream); });
    HostStage hs(ctx);
    const int x = hs.in(view->data, span), o = hs.out(pyr, (size_t)plan->tab.frame_px_out * 3 * 4 * n_frames);
    return hs.run([&] {
        silent_frame_view staged = *view;
        staged.data = hs.dev<uint8_t>(x);
        return with_rgb_view(plan, &staged, n_frames, [&](auto frames) { return launch_pyramid_rgb8(ctx, who, plan, frames, n_frames, hs.dev<float>(o), nullptr); });
    });
}

SILENT_EXPORT int silent_pyramid_rgb8_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                               float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_rgb8_view(ctx, false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_rgb8_view_dev");
}

SILENT_EXPORT int silent_pyramid_rgb8_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                           float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_rgb8_view(ctx, true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_rgb8_view");
}

// The YUV-family colour sources (silent_hip.h; Source<S>, silent_plan.h): NV12 and P010 / P012 / P016 decoder surfaces, planar / packed
// 8-bit YUV, 16-bit YUV.  The struct's own refusals, then the shared ones, all under the entry point's name.  A triple struct that IS
// NV12 / P010 takes the pair kernels (with_yuv).  What the host forms stage: a pair struct exactly the luma span and the chroma span, as
// two inputs; a triple struct the union of its three spans (yuv_stage: a packed buffer once; an interval starts at a plane's address,
// so staged uint16 planes stay 2-byte aligned) -- and the plane pointers are rebased.
template <class S, class F>
static int source_host(silent_ctx* ctx, const S* f, size_t y_span, size_t c_span, int n_frames, void* out, size_t out_bytes, F&& launch) {
    typedef typename Source<S>::elem E;
    HostStage hs(ctx);
    int in[3] = {0, 0, 0}, of[3] = {0, 1, 1};
    size_t delta[3] = {0, 0, 0};
    if constexpr (Source<S>::pair) {
        in[0] = hs.in(f->y, y_span);
        in[1] = hs.in(f->uv, c_span);
    } else {
        const YuvStage st = yuv_stage(f, y_span, c_span);
        for (int i = 0; i < st.n; ++i) in[i] = hs.in(st.start[i], st.bytes[i]);
        for (int k = 0; k < 3; ++k) of[k] = st.of[k], delta[k] = st.delta[k];
    }
    const int o = hs.out(out, out_bytes);
    return hs.run([&] {
        const E* p[3];
        for (int k = 0; k < 3; ++k) p[k] = reinterpret_cast<const E*>(hs.dev<uint8_t>(in[of[k]]) + delta[k]);
        return with_source(f, p, n_frames, [&](auto frames) { return launch(frames, hs.dev<float>(o), (hipStream_t) nullptr); });
    });
}
// f(frames) with the struct's own planes (the _dev forms)
template <class S, class F>
static int source_dev(const S* f, int n_frames, F&& launch) {
    const typename Source<S>::elem* p[3];
    p[0] = f->y;
    if constexpr (Source<S>::pair) p[1] = p[2] = f->uv;
    else p[1] = f->u, p[2] = f->v;
    return with_source(f, p, n_frames, launch);
}

template <class S>
static int pyramid_source(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const S* f, int n_frames, float* pyr, silent_stream stream) {
    const char* who = Source<S>::pyramid;
    size_t y_span = 0, c_span = 0;
    TRY(check_source(ctx, who, plan != nullptr, plan ? plan->tab.H : 0, plan ? plan->tab.W : 0, f, n_frames, &y_span, &c_span));
    TRY(pyramid_checks<float>(ctx, who, plan, true, n_frames, pyr));
    if (plan->tab.C != 3)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": " + Source<S>::noun + " are for 3-channel plans (a single-channel plan reads the luma plane through " +
                                                   (sizeof(typename Source<S>::elem) == 2 ? "silent_pyramid_view16)" : "silent_pyramid_view)"));
    auto launch = [&](auto frames, float* out, hipStream_t s) { return launch_pyramid_rgb8(ctx, who, plan, frames, n_frames, out, s); };
    if (!host) return source_dev(f, n_frames, [&](auto frames) { return launch(frames, pyr, (hipStream_t)stream); });
    return source_host(ctx, f, y_span, c_span, n_frames, pyr, (size_t)plan->tab.frame_px_out * 3 * 4 * n_frames, launch);
}

// the converted frames themselves, [n_frames, H, W, 3] float32 (source_to_rgb_kernel on the frame kind that reads the struct: the
// loaders' own device functions)
template <class S>
static int source_to_rgb(silent_ctx* ctx, bool host, const S* f, int n_frames, int H, int W, float* rgb, silent_stream stream) {
    const char* who = Source<S>::to_rgb;
    size_t y_span = 0, c_span = 0;
    TRY(check_source(ctx, who, true, H, W, f, n_frames, &y_span, &c_span));
    if (!rgb) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_frames must be >= 1");
    const long long per_frame = ((long long)H * W + 255) / 256;
    if (per_frame * n_frames > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many blocks for one launch");
    auto launch = [&](auto frames, float* out, hipStream_t s) {
        typedef typename std::remove_cv<typename std::remove_pointer<decltype(frames)>::type>::type FT;
        hipLaunchKernelGGL(silent::source_to_rgb_kernel<FT>, dim3((unsigned)(per_frame * n_frames)), dim3(256), 0, s, *frames, out, H, W, (int)per_frame);
        (void)frames;
        return check_launch(ctx, who);
    };
    if (!host) return source_dev(f, n_frames, [&](auto frames) { return launch(frames, rgb, (hipStream_t)stream); });
    return source_host(ctx, f, y_span, c_span, n_frames, rgb, (size_t)H * W * 3 * 4 * n_frames, launch);
}

SILENT_EXPORT int silent_pyramid_nv12_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_nv12_frames* frames, int n_frames,
                                          float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_nv12_dev");
}

SILENT_EXPORT int silent_pyramid_nv12(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_nv12_frames* frames, int n_frames,
                                      float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_nv12");
}

SILENT_EXPORT int silent_nv12_to_rgb_dev(silent_ctx* ctx, const silent_nv12_frames* frames, int n_frames, int H, int W, float* rgb,
                                         silent_stream stream) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, false, frames, n_frames, H, W, rgb, stream);
} catch (...) {
    return on_exception(ctx, "silent_nv12_to_rgb_dev");
}

SILENT_EXPORT int silent_nv12_to_rgb(silent_ctx* ctx, const silent_nv12_frames* frames, int n_frames, int H, int W, float* rgb) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, true, frames, n_frames, H, W, rgb, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_nv12_to_rgb");
}

SILENT_EXPORT int silent_pyramid_p010_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_p010_frames* frames, int n_frames,
                                          float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_p010_dev");
}

SILENT_EXPORT int silent_pyramid_p010(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_p010_frames* frames, int n_frames,
                                      float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_p010");
}

SILENT_EXPORT int silent_p010_to_rgb_dev(silent_ctx* ctx, const silent_p010_frames* frames, int n_frames, int H, int W, float* rgb,
                                         silent_stream stream) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, false, frames, n_frames, H, W, rgb, stream);
} catch (...) {
    return on_exception(ctx, "silent_p010_to_rgb_dev");
}

SILENT_EXPORT int silent_p010_to_rgb(silent_ctx* ctx, const silent_p010_frames* frames, int n_frames, int H, int W, float* rgb) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, true, frames, n_frames, H, W, rgb, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_p010_to_rgb");
}

SILENT_EXPORT int silent_pyramid_yuv_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv_frames* frames, int n_frames,
                                         float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_yuv_dev");
}

SILENT_EXPORT int silent_pyramid_yuv(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv_frames* frames, int n_frames,
                                     float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_yuv");
}

SILENT_EXPORT int silent_yuv_to_rgb_dev(silent_ctx* ctx, const silent_yuv_frames* frames, int n_frames, int H, int W, float* rgb,
                                        silent_stream stream) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, false, frames, n_frames, H, W, rgb, stream);
} catch (...) {
    return on_exception(ctx, "silent_yuv_to_rgb_dev");
}

SILENT_EXPORT int silent_yuv_to_rgb(silent_ctx* ctx, const silent_yuv_frames* frames, int n_frames, int H, int W, float* rgb) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, true, frames, n_frames, H, W, rgb, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_yuv_to_rgb");
}

SILENT_EXPORT int silent_pyramid_yuv16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv16_frames* frames, int n_frames,
                                           float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_yuv16_dev");
}

SILENT_EXPORT int silent_pyramid_yuv16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_yuv16_frames* frames, int n_frames,
                                       float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_source(ctx, true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_yuv16");
}

SILENT_EXPORT int silent_yuv16_to_rgb_dev(silent_ctx* ctx, const silent_yuv16_frames* frames, int n_frames, int H, int W, float* rgb,
                                          silent_stream stream) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, false, frames, n_frames, H, W, rgb, stream);
} catch (...) {
    return on_exception(ctx, "silent_yuv16_to_rgb_dev");
}

SILENT_EXPORT int silent_yuv16_to_rgb(silent_ctx* ctx, const silent_yuv16_frames* frames, int n_frames, int H, int W, float* rgb) try {
    NEED_CTX(ctx);
    return source_to_rgb(ctx, true, frames, n_frames, H, W, rgb, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_yuv16_to_rgb");
}

// Raw 8-bit Bayer mosaics (silent_hip.h; check_bayer / bayer_frames, silent_plan.h): the struct's own refusals, then the shared ones, all
// under the entry point's name, before a launch or a staged byte.  The host forms stage the view's span.
static int pyramid_bayer(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const silent_bayer_frames* f, int n_frames, float* pyr, silent_stream stream) {
    const char* who = "silent_pyramid_bayer";
    size_t span = 0;
    TRY(check_bayer(ctx, who, plan != nullptr, plan ? plan->tab.H : 0, plan ? plan->tab.W : 0, f, n_frames, &span));
    TRY(pyramid_checks<float>(ctx, who, plan, true, n_frames, pyr));
    // (a SILENT_PLAN_ACCUM_F64 plan is single-channel by construction: it is named as such, before the channel count)
    if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": Bayer mosaics with a SILENT_PLAN_ACCUM_F64 plan");
    if (plan->tab.C != 3) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": Bayer mosaics are for 3-channel plans");
    auto launch = [&](const uint8_t* data, float* out, hipStream_t s) {
        const Bayer frames = bayer_frames(f, data, n_frames, plan->tab.H, plan->tab.W);
        return launch_pyramid_rgb8(ctx, who, plan, &frames, n_frames, out, s);
    };
    if (!host) return launch(f->data, pyr, (hipStream_t)stream);
    HostStage hs(ctx);
    const int x = hs.in(f->data, span), o = hs.out(pyr, (size_t)plan->tab.frame_px_out * 3 * 4 * n_frames);
    return hs.run([&] { return launch(hs.dev<uint8_t>(x), hs.dev<float>(o), nullptr); });
}

// the converted frames themselves, [n_frames, H, W, 3] float32 (source_to_rgb_kernel: BayerSrc::rgb, the device function of every kernel)
static int bayer_to_rgb(silent_ctx* ctx, bool host, const silent_bayer_frames* f, int n_frames, int H, int W, float* rgb, silent_stream stream) {
    const char* who = "silent_bayer_to_rgb";
    size_t span = 0;
    TRY(check_bayer(ctx, who, true, H, W, f, n_frames, &span));
    if (!rgb) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_frames must be >= 1");
    const long long per_frame = ((long long)H * W + 255) / 256;
    if (per_frame * n_frames > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many blocks for one launch");
    auto launch = [&](const uint8_t* data, float* out, hipStream_t s) {
        hipLaunchKernelGGL(silent::source_to_rgb_kernel<Bayer>, dim3((unsigned)(per_frame * n_frames)), dim3(256), 0, s, bayer_frames(f, data, n_frames, H, W), out,
                           H, W, (int)per_frame);
        return check_launch(ctx, who);
    };
    if (!host) return launch(f->data, rgb, (hipStream_t)stream);
    HostStage hs(ctx);
    const int x = hs.in(f->data, span), o = hs.out(rgb, (size_t)H * W * 3 * 4 * n_frames);
    return hs.run([&] { return launch(hs.dev<uint8_t>(x), hs.dev<float>(o), nullptr); });
}

SILENT_EXPORT int silent_pyramid_bayer_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_bayer_frames* frames, int n_frames,
                                           float* pyr, silent_stream stream) try {
    NEED_CTX(ctx);
    return pyramid_bayer(ctx, false, plan, frames, n_frames, pyr, stream);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_bayer_dev");
}

SILENT_EXPORT int silent_pyramid_bayer(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_bayer_frames* frames, int n_frames,
                                       float* pyr) try {
    NEED_CTX(ctx);
    return pyramid_bayer(ctx, true, plan, frames, n_frames, pyr, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_pyramid_bayer");
}

SILENT_EXPORT int silent_bayer_to_rgb_dev(silent_ctx* ctx, const silent_bayer_frames* frames, int n_frames, int H, int W, float* rgb,
                                          silent_stream stream) try {
    NEED_CTX(ctx);
    return bayer_to_rgb(ctx, false, frames, n_frames, H, W, rgb, stream);
} catch (...) {
    return on_exception(ctx, "silent_bayer_to_rgb_dev");
}

SILENT_EXPORT int silent_bayer_to_rgb(silent_ctx* ctx, const silent_bayer_frames* frames, int n_frames, int H, int W, float* rgb) try {
    NEED_CTX(ctx);
    return bayer_to_rgb(ctx, true, frames, n_frames, H, W, rgb, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_bayer_to_rgb");
}
