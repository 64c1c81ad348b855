// libsilent_hip.so -- pointwise ops, per-level thresholds, 3x3 NMS, keypoint indices, centroids, boosting state and the
// display-graph glue (silent_peaks.h); silent_rgb_keypoints = the fused RGB chain (silent_rgb_api.hip) + the keypoint tail,
// silent_gray_keypoints = the gray pass with its keypoint epilogue (silent_gray_api.hip) + the same tail on K channels.
#include "silent_internal.h"
#include "silent_peaks.h"
#include "silent_peaks_plan.h"
#include "silent_plan.h"

using namespace silent;

// a refusal of the planning (silent_peaks_plan.h) under the entry point's name
static int refuse(silent_ctx* ctx, const char* who, const Refusal& r) {
    return r.status == SILENT_OK ? SILENT_OK : fail(ctx, r.status, std::string(who) + r.tail);
}

// channel counts the fused selection kernels are instantiated for (1, RGB's 3, the gray line-end banks' 4 and 8; a gray bank of
// 3 shares RGB's instantiation)
static bool select_channels_ok(int c) { return c == 1 || c == 3 || c == 4 || c == 8; }
// f(std::integral_constant<int, C>) for the instantiation that serves `channels` (anything but 3, 4, 8: 1)
template <class F>
static void with_channels(int channels, F&& f) {
    if (channels == 3) f(std::integral_constant<int, 3>{});
    else if (channels == 4) f(std::integral_constant<int, 4>{});
    else if (channels == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 1>{});
}

// ------------------------------------------------------------------------------------------ pointwise / nms

SILENT_EXPORT int silent_pad_inwards_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                         int n_frames, int channels, int pt, int pb, int pl, int pr, float* out,
                                         silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_pad_inwards";
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (channels < 1 || pt < 0 || pb < 0 || pl < 0 || pr < 0)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": channels must be >= 1 and paddings >= 0");
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    hipLaunchKernelGGL(pad_inwards_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, tab,
                       channels, pt, pb, pl, pr);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_pad_inwards_dev");
}

// value_from_color / bw_from_color: one body over the two kernels
static int from_color_dev(silent_ctx* ctx, const char* who, void (*kernel)(const float*, float*, long long, int), const float* in,
                          const silent_extent* levels, int n_levels, int n_frames, int channels, float* out, silent_stream stream) {
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": channels must be >= 1");
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    const long long npx = tab.frame_px * n_frames;
    const long long grid = std::min<long long>((npx + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, in, out, npx, channels);
    return check_launch(ctx, who);
}

SILENT_EXPORT int silent_value_from_color_dev(silent_ctx* ctx, const float* in, const silent_extent* levels,
                                              int n_levels, int n_frames, int channels, float* out,
                                              silent_stream stream) try {
    NEED_CTX(ctx);
    return from_color_dev(ctx, "silent_value_from_color", value_from_color_kernel, in, levels, n_levels, n_frames, channels, out, stream);
} catch (...) {
    return on_exception(ctx, "silent_value_from_color_dev");
}

SILENT_EXPORT int silent_bw_from_color_dev(silent_ctx* ctx, const float* in, const silent_extent* levels,
                                              int n_levels, int n_frames, int channels, float* out,
                                              silent_stream stream) try {
    NEED_CTX(ctx);
    return from_color_dev(ctx, "silent_bw_from_color", bw_from_color_kernel, in, levels, n_levels, n_frames, channels, out, stream);
} catch (...) {
    return on_exception(ctx, "silent_bw_from_color_dev");
}

SILENT_EXPORT int silent_nms3x3_dev(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                    int n_frames, int channels, int mode, float* out, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_nms3x3";
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": channels must be >= 1");
    if (mode != SILENT_NMS_PRODUCT && mode != SILENT_NMS_FIRED)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": mode must be SILENT_NMS_PRODUCT or SILENT_NMS_FIRED");
    LevelTab tab;
    long long blocks;
    if (channels == 1 || channels == 3) {  // streaming stencil
        TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kNmsTW, kNmsTH, &tab, &blocks));
        if (channels == 3)
            hipLaunchKernelGGL(nms3x3_stream_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, tab, mode);
        else
            hipLaunchKernelGGL(nms3x3_stream_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, tab, mode);
        return check_launch(ctx, who);
    }
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    hipLaunchKernelGGL(nms3x3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, tab, channels,
                       mode);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_nms3x3_dev");
}

// ------------------------------------------------------------------------------------------ top-percent threshold

SILENT_EXPORT int silent_top_value_points_dev(silent_ctx* ctx, const float* color, const float* value,
                                              const silent_extent* levels, int n_levels, int n_frames, int channels,
                                              double top_percent, float* out, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_top_value_points";
    if (!color || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": channels must be >= 1");
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    LevelTab rtab;
    long long rblocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kRedChunk, 0, &rtab, &rblocks));
    const int nmm = n_frames * n_levels;
    TRY(workspace(ctx, (hipStream_t)stream, sizeof(unsigned) * 2 * (size_t)nmm));
    unsigned* mm = (unsigned*)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(init_maxmin_kernel, dim3((nmm + 255) / 256), dim3(256), 0, s, mm, nmm);
    hipLaunchKernelGGL(level_maxmin_kernel, dim3((unsigned)rblocks), dim3(256), 0, s, value, value ? nullptr : color,
                       channels, rtab, mm);
    // python: (1.0 - top_percent) and top_percent are doubles that TF casts to float32 constants
    const float a = (float)(1.0 - top_percent), b = (float)top_percent;
    hipLaunchKernelGGL(top_value_points_kernel, dim3((unsigned)blocks), dim3(256), 0, s, color, value, out, tab,
                       channels, a, b, mm);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_top_value_points_dev");
}

SILENT_EXPORT int silent_select_peaks_dev(silent_ctx* ctx, const float* color, const float* value,
                                          const silent_extent* levels, int n_levels, int n_frames, int channels,
                                          double top_percent, float* top_out, float* peaks_out, float* peak_value_out,
                                          silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_select_peaks";
    if (!color) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (!top_out && !peaks_out && !peak_value_out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": all outputs are NULL");
    if (!select_channels_ok(channels)) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": channels must be 1, 3, 4 or 8");
    LevelTab rtab, tab;
    long long rblocks, blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kRedChunk, 0, &rtab, &rblocks));
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kSelTW, kSelTH, &tab, &blocks));
    const int nmm = n_frames * n_levels;
    TRY(workspace(ctx, (hipStream_t)stream, sizeof(unsigned) * 2 * (size_t)nmm));
    unsigned* mm = (unsigned*)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(init_maxmin_kernel, dim3((nmm + 255) / 256), dim3(256), 0, s, mm, nmm);
    hipLaunchKernelGGL(level_maxmin_kernel, dim3((unsigned)rblocks), dim3(256), 0, s, value, value ? nullptr : color,
                       channels, rtab, mm);
    const float a = (float)(1.0 - top_percent), b = (float)top_percent;
    RegionTab no_regions;
    std::memset(&no_regions, 0, sizeof(no_regions));
    with_channels(channels, [&](auto C) {
        hipLaunchKernelGGL((select_peaks_kernel<decltype(C)::value, false>), dim3((unsigned)blocks), dim3(256), 0, s, color, value, top_out,
                           peaks_out, peak_value_out, tab, a, b, mm, no_regions, nullptr, nullptr, (unsigned)blocks);
    });
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_select_peaks_dev");
}

// ------------------------------------------------------------------------------------------ keypoint indices

// workspace of the keypoint passes, after `reserve` bytes the caller keeps for itself (the order: keypoint_layout, silent_peaks_plan.h)
struct KeypointWs {
    unsigned* cells;
    int* chunk_counts;
    long long* chunk_offsets;
    size_t n_cells;
    float* m1;       // general path: row maxima over the column windows
    float* pooled;   // general path: window maxima
    unsigned long long* hit_masks;   // 1 bit per pixel: the count pass's ballots, read by the write pass
    // sparse tail (silent_rgb_keypoints without a peak-value map; silent_peaks.h, sparse_select_kernel)
    float* sum = nullptr;            // the chain kernel's value summary (SumTab geometry)
    Candidate* cand = nullptr;       // [n_frames][kCandCap]
    int* cand_n = nullptr;           // [n_frames]
    int* dense_flags = nullptr;      // [n_frames][n_levels]: kTailSparse / kTailDense / kTailZero
    int* nan_flags = nullptr;        // [n_frames][n_levels]: the chain kernel saw a NaN value in that level
    float* pv = nullptr;             // peak-value map of the (frame, level)s that run the dense kernels
    void* zero_from = nullptr;       // chunk_counts | hit_masks | cand_n | nan flags: one memset before a sparse tail's chain launch
    size_t zero_bytes = 0;
};

// general path: window maxima of every level into w.pooled (two launches)
static int region_window_maxima(silent_ctx* ctx, const char* who, const float* value, const silent_extent* levels, int n_levels,
                                int n_frames, const RegionTab& rt, const KeypointWs& w, hipStream_t s) {
    LevelTab rowtab;
    long long rows;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 1 << 30, 1, &rowtab, &rows));   // one tile per row
    long long cols = 0;
    for (int l = 0; l < n_levels; ++l) cols += rt.lv[l].ow;
    hipLaunchKernelGGL(region_rowmax_kernel, dim3((unsigned)rows), dim3(256), 0, s, value, rowtab, rt, w.m1);
    const long long threads = cols * n_frames;
    hipLaunchKernelGGL(region_colmax_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, w.m1, rowtab, rt, n_frames,
                       cols, w.pooled);
    return check_launch(ctx, who);
}

// Blocks of a sparse-tail launch over n tiles whose blocks mostly find nothing to do (for_live_tiles, silent_peaks.h): a block
// looks at up to 64 tiles; 2048 blocks keep the chip busy where a frame does run the dense kernels.
static unsigned sparse_grid(long long n) { return (unsigned)std::min<long long>(n, std::max<long long>((n + 63) / 64, 2048)); }

// count -> scan -> ordered write, given the cell maxima
static void keypoint_passes(const float* value, const LevelTab& tab, long long blocks, const RegionTab& rt, const KeypointWs& w,
                            bool general, int n_frames, int64_t* idx, size_t cap_per_frame, int64_t* counts, hipStream_t s,
                            const int* dense_flags = nullptr, float* caller_map = nullptr) {
    if (general)
        hipLaunchKernelGGL(region_count_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, value, tab, rt, w.cells, w.pooled, w.chunk_counts, w.hit_masks, dense_flags);
    else
        hipLaunchKernelGGL(region_count_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, value, tab, rt, w.cells, w.pooled, w.chunk_counts, w.hit_masks, dense_flags);
    if (dense_flags)   // sparse tail: the candidates' hits join what the count pass left, then the scan (one block per frame both)
        hipLaunchKernelGGL(sparse_finish_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, tab, rt, w.cells, w.cand, w.cand_n, dense_flags,
                           w.hit_masks, w.chunk_counts, caller_map, w.chunk_offsets, counts);
    else
        hipLaunchKernelGGL(region_scan_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, w.chunk_counts, w.chunk_offsets,
                           tab.tiles_per_frame, counts);
    if (!cap_per_frame) return;
    hipLaunchKernelGGL(region_write_kernel, dim3((unsigned)blocks), dim3(256), 0, s, tab, w.hit_masks, w.chunk_offsets, idx,
                       (long long)cap_per_frame, w.chunk_counts);
}

// a-11 in two halves: tables + workspace (after `reserve` bytes the caller keeps at the head of the workspace), then the passes --
// so that silent_gray_keypoints can write the value map into the reserved bytes in between
struct RegionPlan {
    LevelTab tab, ctab;
    long long blocks, cblocks;
    RegionTab rt;
    bool general;
    KeypointWs w;
};

static int keypoint_workspace(silent_ctx* ctx, hipStream_t stream, int n_levels, int n_frames, size_t reserve, RegionPlan* rp,
                              long long sum_entries = 0, long long pv_px = 0) {
    const KeypointLayout k = keypoint_layout(n_levels, n_frames, rp->blocks, reserve, rp->rt, rp->general, sum_entries, pv_px);
    TRY(workspace(ctx, stream, k.total));
    char* base = (char*)ctx->ws.p;
    KeypointWs* w = &rp->w;
    w->n_cells = k.n_cells;
    w->cells = (unsigned*)(base + k.cells);
    w->chunk_counts = (int*)(base + k.chunk_counts);
    w->hit_masks = (unsigned long long*)(base + k.hit_masks);
    w->cand_n = (int*)(base + k.cand_n);
    w->nan_flags = (int*)(base + k.nan_flags);
    w->chunk_offsets = (long long*)(base + k.chunk_offsets);
    w->m1 = (float*)(base + k.m1);
    w->pooled = (float*)(base + k.pooled);
    w->sum = sum_entries ? (float*)(base + k.sum) : nullptr;
    w->cand = sum_entries ? (Candidate*)(base + k.cand) : nullptr;
    w->dense_flags = (int*)(base + k.dense_flags);
    w->pv = pv_px ? (float*)(base + k.pv) : nullptr;
    w->zero_from = base + k.zero_from;
    w->zero_bytes = k.zero_bytes;
    return SILENT_OK;
}

static int region_tables(silent_ctx* ctx, const char* who, const silent_extent* levels, int n_levels, int n_frames,
                         const silent_extent* regions, RegionPlan* rp) {
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kKpChunk, 0, &rp->tab, &rp->blocks));     // count / write chunks
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kRedChunk, 0, &rp->ctab, &rp->cblocks));  // cell maxima, per-level extrema
    return refuse(ctx, who, build_region_tab(levels, n_levels, regions, &rp->rt, &rp->general));
}

static int region_prepare(silent_ctx* ctx, const char* who, const silent_extent* levels, int n_levels, int n_frames,
                          const silent_extent* regions, size_t reserve, hipStream_t s, RegionPlan* rp) {
    TRY(region_tables(ctx, who, levels, n_levels, n_frames, regions, rp));
    return keypoint_workspace(ctx, s, n_levels, n_frames, reserve, rp);
}

static int region_run(silent_ctx* ctx, const char* who, const float* value, const silent_extent* levels, int n_levels, int n_frames,
                      const RegionPlan& rp, int64_t* idx, size_t cap_per_frame, int64_t* counts, hipStream_t s) {
    const KeypointWs& w = rp.w;
    if (rp.general) {
        TRY(region_window_maxima(ctx, who, value, levels, n_levels, n_frames, rp.rt, w, s));
    } else {
        hipLaunchKernelGGL(init_cells_kernel, dim3((unsigned)((w.n_cells + 255) / 256)), dim3(256), 0, s, w.cells, (long long)w.n_cells);
        hipLaunchKernelGGL(region_cell_max_kernel, dim3((unsigned)rp.cblocks), dim3(256), 0, s, value, rp.ctab, rp.rt, w.cells);
    }
    keypoint_passes(value, rp.tab, rp.blocks, rp.rt, w, rp.general, n_frames, idx, cap_per_frame, counts, s);
    return check_launch(ctx, who);
}

SILENT_EXPORT int silent_max_value_indices_region_dev(silent_ctx* ctx, const float* value, const silent_extent* levels,
                                                      int n_levels, int n_frames, const silent_extent* regions,
                                                      int64_t* idx, size_t cap_per_frame, int64_t* counts,
                                                      silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_max_value_indices_region";
    if (!value || !regions || !counts || (!idx && cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    RegionPlan rp;
    TRY(region_prepare(ctx, who, levels, n_levels, n_frames, regions, 0, (hipStream_t)stream, &rp));
    return region_run(ctx, who, value, levels, n_levels, n_frames, rp, idx, cap_per_frame, counts, (hipStream_t)stream);
} catch (...) {
    return on_exception(ctx, "silent_max_value_indices_region_dev");
}

// SURVEY 8d config 3 as one call: top-percent -> NMS -> value -> per-region keypoint indices of the peak value.
// = silent_select_peaks + silent_max_value_indices_region, with the cell maxima folded into the selection pass.
// Two halves so that silent_rgb_keypoints can run the chain kernel in between (it fills the per-level extrema itself).
struct SelectPlan : RegionPlan {   // (ctab also serves the reduction pass of the per-level extrema)
    LevelTab stab;  // the selection pass's tiles
    long long sblocks;
    unsigned* mm;   // [n_frames][n_levels][2] ordered-uint extrema, at the head of the context workspace
    int nmm;
    SumTab st;      // sparse tail: geometry of the chain kernel's value summary (frame_entries = 0: none)
    float* value_ws = nullptr;   // a float32 value map behind the extrema (select_prepare's value_px), for a caller that passes none
};

// tables, workspace, and the init kernels.  sparse_th > 0: also lay out the sparse tail for a chain launch with that tile
// height; pv_ws: keep room for a peak-value map in the workspace (the caller has none)
static int select_prepare(silent_ctx* ctx, const char* who, const silent_extent* levels, int n_levels, int n_frames,
                          const silent_extent* regions, hipStream_t s, SelectPlan* sp, int sparse_th = 0, bool pv_ws = false,
                          bool value_ws = false) {
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, kSelTW, kSelTH, &sp->stab, &sp->sblocks));
    TRY(region_tables(ctx, who, levels, n_levels, n_frames, regions, sp));
    sp->nmm = n_frames * n_levels;
    build_sum_tab(levels, n_levels, n_frames, sparse_th, sp->general, &sp->st);
    // the head the caller keeps: the extrema, then (value_ws) a whole float32 value map
    const size_t mm_bytes = sizeof(unsigned) * 2 * (size_t)sp->nmm;
    const size_t head = value_ws ? align_up(mm_bytes) + (size_t)sp->tab.frame_px * n_frames * sizeof(float) : mm_bytes;
    TRY(keypoint_workspace(ctx, s, n_levels, n_frames, head, sp, sp->st.frame_entries, pv_ws ? sp->tab.frame_px : 0));
    sp->mm = (unsigned*)ctx->ws.p;
    sp->value_ws = value_ws ? (float*)((char*)ctx->ws.p + align_up(mm_bytes)) : nullptr;
    const long long n_init = std::max<long long>(2ll * sp->nmm, (long long)sp->w.n_cells);
    const long long n_zero16 = sp->st.frame_entries > 0 ? (long long)(sp->w.zero_bytes / 16) : 0;   // (every piece of the workspace is align_up'ed)
    const long long init_blocks = std::max((n_init + 255) / 256, std::min<long long>((n_zero16 + 255) / 256, 8ll * ctx->n_cus));
    hipLaunchKernelGGL(init_select_kernel, dim3((unsigned)init_blocks), dim3(256), 0, s, sp->mm, 2 * sp->nmm, sp->w.cells,
                       (long long)sp->w.n_cells, (uint4*)sp->w.zero_from, n_zero16);
    return SILENT_OK;
}

// The selection launches of select_run for C channels; PAD: `color` is unpadded, pad_inwards' mask is applied as it is read
// (silent_gray_keypoints).  sparse_pass: sparse_select_kernel; otherwise the streaming selection pass.
template <int C, bool PAD, typename CT>
static void select_launches(const SelectPlan& sp, bool sparse_pass, const CT* color, const float* value, float* pv_map, float a,
                            float b, const int* dense_flags, int n_frames, int pad, hipStream_t s) {
    const RegionTab& rt = sp.rt;
    const KeypointWs& w = sp.w;
    if (sparse_pass) {
        hipLaunchKernelGGL((sparse_select_kernel<C, PAD, CT>), dim3((unsigned)((sp.st.frame_entries + 255) / 256), (unsigned)n_frames), dim3(256), 0, s,
                           color, sp.tab, sp.st, w.sum, n_frames, a, b, sp.mm, rt, w.cells, w.cand, w.cand_n, pad, value);
    } else if (sp.general) {
        // many windows: the selection pass without the folded cell maxima (the separable window maxima follow)
        hipLaunchKernelGGL((select_peaks_kernel<C, false, PAD, CT>), dim3((unsigned)sp.sblocks), dim3(256), 0, s, color, value, nullptr, nullptr,
                           pv_map, sp.stab, a, b, sp.mm, rt, nullptr, nullptr, (unsigned)sp.sblocks, pad);
    } else {
        // (sparse tail: a bounded grid -- usually no (frame, level) runs this pass)
        hipLaunchKernelGGL((select_peaks_kernel<C, true, PAD, CT>), dim3(dense_flags ? sparse_grid(sp.sblocks) : (unsigned)sp.sblocks), dim3(256), 0, s,
                           color, value, nullptr, nullptr, pv_map, sp.stab, a, b, sp.mm, rt, w.cells, dense_flags, (unsigned)sp.sblocks, pad);
    }
}

// have_mm: the extrema are already in sp.mm (no reduction pass).  sparse: the chain kernel left its value summary in sp.w.sum
// (geometry sp.st) -- the sparse tail runs and the dense kernels only where it could not settle a (frame, level).  pad > 0: `color`
// is the unpadded map of silent_gray_keypoints (select_launches); the extrema must then be present (have_mm).
// CT = _Float16 (silent_rgb_keypoints_h): `color` is the float16 line_end map, widened where it is loaded; `value` is then required
// (the float32 value map: every comparison with the threshold reads it), channels = 3, pad = 0.
template <typename CT>
static int select_run(silent_ctx* ctx, const char* who, const CT* color, const float* value, const silent_extent* levels,
                      int n_levels, int n_frames, int channels, double top_percent, const SelectPlan& sp, bool have_mm,
                      float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts, hipStream_t s,
                      bool sparse = false, int pad = 0) {
    unsigned* mm = sp.mm;
    const RegionTab& rt = sp.rt;
    const KeypointWs& w = sp.w;
    if (!have_mm)
        hipLaunchKernelGGL(level_maxmin_kernel, dim3((unsigned)sp.cblocks), dim3(256), 0, s, value,
                           value ? nullptr : reinterpret_cast<const float*>(color) /* (CT = float: a float16 map comes with its value map) */,
                           channels, sp.ctab, mm);
    const float a = (float)(1.0 - top_percent), b = (float)top_percent;
    const int* dense_flags = nullptr;
    float* const caller_map = peak_value_out;
    auto launches = [&](bool sparse_pass, float* pv_map) {
        if constexpr (!std::is_same<CT, float>::value) {
            select_launches<3, false, CT>(sp, sparse_pass, color, value, pv_map, a, b, dense_flags, n_frames, 0, s);
        } else {
        with_channels(channels, [&](auto C) {
            if (pad > 0) select_launches<decltype(C)::value, true, float>(sp, sparse_pass, color, value, pv_map, a, b, dense_flags, n_frames, pad, s);
            else select_launches<decltype(C)::value, false, float>(sp, sparse_pass, color, value, pv_map, a, b, dense_flags, n_frames, pad, s);
        });
        }
    };
    if (sparse) {
        // (sparse implies: cell tables, extrema present; select_prepare zeroed the counters)
        launches(true, nullptr);
        hipLaunchKernelGGL(sparse_modes_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, sp.tab, rt, w.cells, w.cand_n, w.nan_flags,
                           w.dense_flags, peak_value_out ? 1 : 0);
        if (peak_value_out)   // the map the caller takes: zeros wherever the dense pass will not write
            hipLaunchKernelGGL(sparse_fill_map_kernel, dim3((unsigned)sp.blocks), dim3(256), 0, s, sp.tab, w.dense_flags, peak_value_out);
        dense_flags = w.dense_flags;
    }
    if (!peak_value_out) peak_value_out = w.pv;
    launches(false, peak_value_out);
    if (sp.general) TRY(region_window_maxima(ctx, who, peak_value_out, levels, n_levels, n_frames, rt, w, s));
    keypoint_passes(peak_value_out, sp.tab, sp.blocks, rt, w, sp.general, n_frames, idx, cap_per_frame, counts, s, dense_flags,
                    dense_flags ? caller_map : nullptr);
    return check_launch(ctx, who);
}

SILENT_EXPORT int silent_select_keypoints_dev(silent_ctx* ctx, const float* color, const float* value,
                                              const silent_extent* levels, int n_levels, int n_frames, int channels,
                                              double top_percent, const silent_extent* regions, float* peak_value_out,
                                              int64_t* idx, size_t cap_per_frame, int64_t* counts, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_select_keypoints";
    if (!color || !regions || !counts || (!idx && cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (!select_channels_ok(channels)) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": channels must be 1, 3, 4 or 8");
    SelectPlan sp;
    TRY(select_prepare(ctx, who, levels, n_levels, n_frames, regions, (hipStream_t)stream, &sp, 0, !peak_value_out));
    return select_run(ctx, who, color, value, levels, n_levels, n_frames, channels, top_percent, sp, false, peak_value_out, idx,
                      cap_per_frame, counts, (hipStream_t)stream);
} catch (...) {
    return on_exception(ctx, "silent_select_keypoints_dev");
}

// ------------------------------------------------------------------------------------------ centroids

SILENT_EXPORT int silent_centroids_dev(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels,
                                       int n_frames, int region_h, int region_w, float* dist_out, float* total_out,
                                       silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_centroids";
    if (!value || !dist_out || !total_out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    CellTab ct;
    TRY(refuse(ctx, who, build_cell_tab(levels, n_levels, region_h, region_w, &ct)));
    const long long cells = ct.frame_cells * n_frames;
    if ((cells + 255) / 256 > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many cells");
    TRY(workspace(ctx, (hipStream_t)stream, (size_t)cells * 2 * sizeof(float)));
    float* cxy = (float*)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(centroid_cells_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, value, tab, ct, n_frames,
                       total_out, cxy);
    hipLaunchKernelGGL(centroid_dist_kernel, dim3((unsigned)blocks), dim3(256), 0, s, tab, ct, cxy, dist_out);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_centroids_dev");
}

// ------------------------------------------------------------------------------------------ boosting state

SILENT_EXPORT int silent_boosting_step_dev(silent_ctx* ctx, const float* input, const silent_extent* levels,
                                           int n_levels, int n_frames, const silent_boosting_params* params,
                                           float* energy, float* fired_out, float* energy_out, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_boosting_step";
    if (!input || !energy || !fired_out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    BoostP bp;
    TRY(refuse(ctx, "silent_boosting_step", boost_params(params, &bp)));
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    const long long n = tab.frame_px * n_frames;
    if ((n + 255) / 256 > 0x7fffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many pixels");
    TRY(workspace(ctx, (hipStream_t)stream, (size_t)n * sizeof(float)));
    float* m = (float*)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(boost_power_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, input, energy, m, n);
    hipLaunchKernelGGL(boost_update_kernel, dim3((unsigned)blocks), dim3(256), 0, s, input, m, energy, fired_out,
                       energy_out, tab, bp);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_boosting_step_dev");
}

// ------------------------------------------------------------------------------------------ display-graph glue

SILENT_EXPORT int silent_affine_clip_dev(silent_ctx* ctx, const float* in, size_t n_values,
                                         const silent_affine_params* params, float* out, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_affine_clip";
    if (!in || !out || !params) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (n_values == 0) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": empty tensor");
    if ((n_values + 2047) / 2048 > 0x7fffffffull) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": too many values");
    const AffineP ap = {params->mul, params->div, params->add, params->lo, params->hi, params->post_add};
    hipLaunchKernelGGL(affine_clip_kernel, dim3((unsigned)((n_values + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream,
                       in, out, (long long)n_values, ap);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_affine_clip_dev");
}

// f(TypeTag<T>) for the element type of a SILENT_DT_*; false: no such dtype (f was not called)
template <class T>
struct TypeTag { using type = T; };
template <class F>
static bool with_dtype(int dt, F&& f) {
    switch (dt) {
        case SILENT_DT_U8: f(TypeTag<unsigned char>{}); return true;
        case SILENT_DT_F32: f(TypeTag<float>{}); return true;
        case SILENT_DT_F64: f(TypeTag<double>{}); return true;
        case SILENT_DT_I32: f(TypeTag<int>{}); return true;
        case SILENT_DT_U16: f(TypeTag<unsigned short>{}); return true;
        case SILENT_DT_I16: f(TypeTag<short>{}); return true;
        case SILENT_DT_I64: f(TypeTag<long long>{}); return true;
        default: return false;
    }
}

static size_t dtype_size(int dt) {
    size_t bytes = 0;   // (0: no such dtype)
    (void)with_dtype(dt, [&](auto tag) { bytes = sizeof(typename decltype(tag)::type); });
    return bytes;
}

SILENT_EXPORT int silent_cast_interleave_dev(silent_ctx* ctx, const void* in, int in_dtype, size_t n_pixels, int in_stride,
                                             int in_offset, int count, float* out, int out_stride, int out_offset,
                                             silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_cast_interleave";
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (!dtype_size(in_dtype)) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": unknown in_dtype");
    if (n_pixels == 0) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": empty tensor");
    if (count < 1 || in_offset < 0 || out_offset < 0 || in_stride < in_offset + count || out_stride < out_offset + count)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": need 0 <= offset and offset + count <= stride on both sides");
    const long long total = (long long)n_pixels * count;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 256ll * 64);
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)n_pixels;
    (void)with_dtype(in_dtype, [&](auto tag) {   // (an unknown dtype was refused above)
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(cast_interleave_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)in, out, n, in_stride, in_offset, count, out_stride, out_offset);
    });
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_cast_interleave_dev");
}

// (silent_displayer_api.hip) np.asarray(frame, float32) for the rectangle of the frame the displayer's pyramid reads
int cast_rect_launch(silent_ctx* ctx, const void* in, int in_dtype, int W, int C, int y0, int x0, int h, int w, float* out, hipStream_t s) {
    const char* who = "silent_displayer_step";
    if (!in || !out || h < 1 || w < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": bad cast rectangle");
    const long long total = (long long)h * w * C;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 256ll * 64);
    const bool known = with_dtype(in_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(cast_rect_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)in, out, W, C, y0, x0, h, w);
    });
    if (!known) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": frame dtype");
    return check_launch(ctx, who);
}

SILENT_EXPORT int silent_resize_nearest_dev(silent_ctx* ctx, const float* in, const silent_extent* in_levels,
                                            int n_levels, int n_frames, int channels, const silent_extent* out_levels,
                                            float* out, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_resize_nearest";
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": channels must be >= 1");
    LevelTab tab;
    long long blocks;
    TRY(build_level_tab(ctx, who, in_levels, n_levels, n_frames, 0, 0, &tab, &blocks));   // validates the input side
    TRY(build_level_tab(ctx, who, out_levels, n_levels, n_frames, 0, 0, &tab, &blocks));
    ResizeTab rt;
    std::memset(&rt, 0, sizeof(rt));
    long long off = 0;
    for (int l = 0; l < n_levels; ++l) {
        rt.ih[l] = in_levels[l].h;
        rt.iw[l] = in_levels[l].w;
        rt.in_off[l] = off;
        off += (long long)in_levels[l].h * in_levels[l].w;
        rt.yscale[l] = (float)in_levels[l].h / (float)out_levels[l].h;
        rt.xscale[l] = (float)in_levels[l].w / (float)out_levels[l].w;
    }
    rt.in_px = off;
    hipLaunchKernelGGL(resize_nearest_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, tab, rt,
                       channels);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_resize_nearest_dev");
}

// ------------------------------------------------------------------------------------------ the displayer's fused tail
// (silent_displayer_api.hip) value [L, h, w] -> the four small results + the advanced state, in two launches (silent_peaks.h, DispTail);
// seq / flag: the frame's completion signal, one launch behind them (NULL: none)
int displayer_tail(silent_ctx* ctx, int L, int h, int w, int rh, int rw, int h2, int w2, const silent_boosting_params* boost, const float* value,
                   float* imp, float* energy, float* out1, float* out2, float* out3, float* update, hipStream_t s, unsigned long long* seq,
                   unsigned long long* flag) {
    const char* who = "silent_displayer_step";
    DispTail t;
    std::memset(&t, 0, sizeof(t));
    TRY(refuse(ctx, "silent_boosting_step", boost_params(boost, &t.bp)));
    const silent_extent full = {h, w}, half = {h2, w2};
    CellTab c1, c2;
    TRY(refuse(ctx, who, build_cell_tab(&full, 1, rh, rw, &c1)));
    TRY(refuse(ctx, who, build_cell_tab(&half, 1, rh, rw, &c2)));
    t.L = L; t.h = h; t.w = w; t.h2 = h2; t.w2 = w2; t.rh = rh; t.rw = rw;
    t.ch = c1.oh[0]; t.cw = c1.ow[0]; t.ch2 = c2.oh[0]; t.cw2 = c2.ow[0];
    t.y_first = c1.y_first[0]; t.x_first = c1.x_first[0]; t.y_first2 = c2.y_first[0]; t.x_first2 = c2.x_first[0];
    t.yscale_c = c1.yscale[0]; t.xscale_c = c1.xscale[0]; t.yscale_c2 = c2.yscale[0]; t.xscale_c2 = c2.xscale[0];
    t.yscale_r = (float)h / (float)h2;      // (silent_resize_nearest_dev: float32 in / out)
    t.xscale_r = (float)w / (float)w2;
    tail_affines(&t);
    const long long px = (long long)L * h * w, px2 = (long long)L * h2 * w2, cells = (long long)L * t.ch * t.cw, cells2 = (long long)L * t.ch2 * t.cw2;
    TRY(workspace(ctx, s, (size_t)(cells * 2 + cells2 * 2 + cells) * sizeof(float)));
    t.cxy = (float*)ctx->ws.p;
    t.cxy2 = t.cxy + cells * 2;
    t.m = t.cxy2 + cells2 * 2;
    t.value = value; t.imp_out = imp; t.energy = energy;
    t.out1 = out1; t.out2 = out2; t.out3 = out3; t.update = update;
    auto grid = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
    hipLaunchKernelGGL(disp_cells_kernel, grid(cells + cells2), dim3(256), 0, s, t);
    hipLaunchKernelGGL(disp_dist_boost_kernel, grid(px + px2 + cells), dim3(256), 0, s, t);
    if (flag) hipLaunchKernelGGL(disp_signal_kernel, dim3(1), dim3(64), 0, s, seq, flag);
    return check_launch(ctx, who);
}

// ------------------------------------------------------------------------------------------ the attention tail of a batch
// (silent_peaks.h, AttnTab; the planning: silent_peaks_plan.h, attention_plan)

SILENT_EXPORT int silent_attention_extents(const silent_extent* levels, int n_levels, const silent_attention_params* p, silent_extent* cells,
                                           silent_extent* half, silent_extent* cells2) try {
    const char* who = "silent_attention_extents";
    if (!p) return fail(nullptr, SILENT_E_INVALID, std::string(who) + ": NULL params");
    return refuse(nullptr, who, attention_extents(levels, n_levels, p->region_h, p->region_w, p->resize_div, cells, half, cells2));
} catch (...) {
    return on_exception(nullptr, "silent_attention_extents");
}

SILENT_EXPORT int silent_attention_tail_dev(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels, int n_frames,
                                            const silent_attention_params* params, float* energy, float* centroids_out,
                                            float* centroids2_out, float* fired_out, float* update_out, silent_stream stream) try {
    NEED_CTX(ctx);
    const char* who = "silent_attention_tail";
    if (!value || !energy || !params) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer (value, energy and params are required)");
    AttnPlan ap;
    TRY(refuse(ctx, who, attention_plan(levels, n_levels, n_frames, params, centroids_out != nullptr, centroids2_out != nullptr, &ap)));
    hipStream_t s = (hipStream_t)stream;
    TRY(workspace(ctx, s, ap.ws.total));
    char* ws = (char*)ctx->ws.p;
    AttnPtr p;
    p.value = value;
    p.energy = energy;
    p.cxy = (float*)(ws + ap.ws.cxy);
    p.cxy2 = (float*)(ws + ap.ws.cxy2);
    p.imp = (float*)(ws + ap.ws.imp);
    p.m = (float*)(ws + ap.ws.m);
    p.out1 = centroids_out;
    p.out2 = centroids2_out;
    p.fired = fired_out;
    p.update = update_out;
    hipLaunchKernelGGL(attn_cells_kernel, dim3((unsigned)((ap.n_cells + ap.n_cells2 + 255) / 256)), dim3(256), 0, s, ap.t, p);
    hipLaunchKernelGGL(attn_pixels_kernel, dim3((unsigned)(ap.px_blocks + ap.px2_blocks + ap.cell_blocks)), dim3(256), 0, s, ap.t, p);
    return check_launch(ctx, who);
} catch (...) {
    return on_exception(ctx, "silent_attention_tail_dev");
}

SILENT_EXPORT int silent_attention_tail(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels, int n_frames,
                                        const silent_attention_params* params, float* energy, float* centroids_out, float* centroids2_out,
                                        float* fired_out, float* update_out) try {
    NEED_CTX(ctx);
    const char* who = "silent_attention_tail";
    if (!value || !energy || !params) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer (value, energy and params are required)");
    AttnPlan ap;   // (the sizes of the staged buffers; the _dev form plans again)
    TRY(refuse(ctx, who, attention_plan(levels, n_levels, n_frames, params, centroids_out != nullptr, centroids2_out != nullptr, &ap)));
    const size_t nf = (size_t)n_frames, cells = (size_t)ap.t.ct1.frame_cells * nf * 4, c = ap.t.bp.visualize ? 3 : 1;
    HostStage hs(ctx);
    const int v = hs.in(value, (size_t)ap.frame_px * nf * 4), e = hs.inout(energy, cells), o1 = hs.out(centroids_out, (size_t)ap.frame_px * nf * 4),
              o2 = hs.out(centroids2_out, (size_t)ap.frame_px2 * nf * 4), f = hs.out(fired_out, cells * c), u = hs.out(update_out, cells * c);
    return hs.run([&] {
        return silent_attention_tail_dev(ctx, hs.dev<float>(v), levels, n_levels, n_frames, params, hs.dev<float>(e), hs.dev<float>(o1),
                                         hs.dev<float>(o2), hs.dev<float>(f), hs.dev<float>(u), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_attention_tail");
}

// ------------------------------------------------------------------------------------------ RGB chain + keypoints

// what silent_sparse_tail_stats reads back of the call that just laid its tail out: whether it ran sparse, where its flags / counters live
static void publish_sparse_tail(silent_ctx* ctx, const SelectPlan& sp, hipStream_t s, int n_frames, int n_levels, bool sparse) {
    ctx->sparse_ran = sparse;
    ctx->sparse_stream = s;
    ctx->sparse_flags_off = (size_t)((char*)sp.w.dense_flags - (char*)ctx->ws.p);
    ctx->sparse_candn_off = (size_t)((char*)sp.w.cand_n - (char*)ctx->ws.p);
    ctx->sparse_pairs = n_frames * n_levels;
    ctx->sparse_frames = n_frames;
}

// Config 3 from the pyramid on in one call: silent_rgb_line_end + silent_select_keypoints on its line_end / value maps.
// When the chain runs as the pair kernel's two-group instantiation, that kernel also accumulates the per-level extrema of the
// value map (a-10's max / min), so the reduction pass is skipped and nobody needs the value map in memory: the selection pass
// takes the value from line_end (same three operations, same bits) and the map is written only if the caller asks for it.
// MT: the element type of the orient / line_end maps -- float (silent_rgb_keypoints), or uint16_t = IEEE binary16 bits
// (silent_rgb_keypoints_h: the chain stores them as float16, the tail widens line_end where it loads it and compares the FLOAT32
// value map with the threshold, so the value map exists -- the caller's, or one in the workspace)
template <typename MT>
static int rgb_keypoints_dev(silent_ctx* ctx, const char* who, const float* pyr, const silent_extent* levels, int n_levels,
                             int n_frames, const silent_rgb_chain_params* p, double top_percent,
                             const silent_extent* regions, MT* orient_out, MT* line_end_out,
                             float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame,
                             int64_t* counts, silent_stream stream) {
    constexpr bool half16 = !std::is_same<MT, float>::value;
    if (!pyr || !p || !regions || !line_end_out || !counts || (!idx && cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (!p->rgc || !p->rgby || !p->stripe || !p->blur || !p->end)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": a kernel pointer in params is NULL");
    bool uniform_blur = true;   // anything else makes the chain use the context workspace itself: plain sequence then
    for (int t = 0; t < 49 && uniform_blur; ++t)
        for (int io = 1; io < 9; ++io)
            if (p->blur[t * 9 + io] != p->blur[t * 9]) uniform_blur = false;
    hipStream_t s = (hipStream_t)stream;
    if (!levels || n_levels < 1 || n_levels > kMaxLevels || n_frames < 1)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": bad levels / n_frames");
    for (int l = 0; l < n_levels; ++l)
        if (levels[l].h < 1 || levels[l].w < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": bad level extent");
    if (!uniform_blur) {
        if constexpr (half16) {   // the launch's own refusal, the only one: the staged route writes float32 maps
            return rgb_chain_launch(ctx, who, pyr, levels, n_levels, n_frames, p, orient_out, line_end_out, value_out, nullptr, nullptr, stream,
                                    nullptr, nullptr, nullptr, true);
        } else {
            TRY(rgb_chain_launch(ctx, who, pyr, levels, n_levels, n_frames, p, orient_out, line_end_out, value_out, nullptr, nullptr, stream));
            return silent_select_keypoints_dev(ctx, line_end_out, value_out, levels, n_levels, n_frames, 3, top_percent, regions,
                                               peak_value_out, idx, cap_per_frame, counts, stream);
        }
    }
    // Without a caller-side peak-value map the tail runs sparse (silent_peaks.h, sparse_select_kernel): the chain kernel leaves
    // a per-group maximum of the value map, and selection / NMS / keypoint search look only at the groups that reach their
    // level's threshold; whatever that cannot settle exactly runs the dense kernels on a map in the workspace.
    bool pair_kernel = false;
    const int th = rgb_chain_tile_height(ctx, levels, n_levels, n_frames, &pair_kernel, true, half16);
    if (half16 && !pair_kernel)   // (the chain launch's refusal, before the tail lays out a workspace for such a level)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": a level is too large for the pair kernel's addressing (float16 storage has no other kernel)");
    // (float16: a line_end above 65504 is stored as +inf, and inf * 0 is a NaN peak value at a pixel whose VALUE is no NaN -- the
    // sparse tail places NaNs by the value map's NaN flags only, so such a clip bound keeps the dense kernels)
    const bool want_sparse = pair_kernel && !(ctx->tune[SILENT_TUNE_RGB] & 32u) && (!half16 || p->clip_hi <= 65504.0f);
    SelectPlan sp;
    TRY(select_prepare(ctx, who, levels, n_levels, n_frames, regions, s, &sp, want_sparse ? th : 0, !peak_value_out, half16 && !value_out));
    if (half16 && !value_out) value_out = sp.value_ws;
    bool mm_done = false;
    TRY(rgb_chain_launch(ctx, who, pyr, levels, n_levels, n_frames, p, orient_out, line_end_out, value_out, sp.mm, &mm_done, stream,
                         &sp.st, sp.w.sum, sp.w.nan_flags, half16));
    const bool sparse = want_sparse && mm_done && sp.st.frame_entries > 0;
    publish_sparse_tail(ctx, sp, s, n_frames, n_levels, sparse);
    if constexpr (half16)
        return select_run(ctx, who, reinterpret_cast<const _Float16*>(line_end_out), value_out, levels, n_levels, n_frames, 3, top_percent, sp,
                          mm_done, peak_value_out, idx, cap_per_frame, counts, s, sparse);
    else
        return select_run(ctx, who, line_end_out, mm_done ? nullptr : value_out, levels, n_levels, n_frames, 3, top_percent, sp, mm_done,
                          peak_value_out, idx, cap_per_frame, counts, s, sparse);
}

SILENT_EXPORT int silent_rgb_keypoints_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                                           int n_frames, const silent_rgb_chain_params* p, double top_percent,
                                           const silent_extent* regions, float* orient_out, float* line_end_out,
                                           float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame,
                                           int64_t* counts, silent_stream stream) try {
    NEED_CTX(ctx);
    return rgb_keypoints_dev<float>(ctx, "silent_rgb_keypoints", pyr, levels, n_levels, n_frames, p, top_percent, regions, orient_out,
                                    line_end_out, value_out, peak_value_out, idx, cap_per_frame, counts, stream);
} catch (...) {
    return on_exception(ctx, "silent_rgb_keypoints_dev");
}

SILENT_EXPORT int silent_rgb_keypoints_h_dev(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                                             int n_frames, const silent_rgb_chain_params* p, double top_percent,
                                             const silent_extent* regions, uint16_t* orient_out, uint16_t* line_end_out,
                                             float* value_out, float* peak_value_out, int64_t* idx, size_t cap_per_frame,
                                             int64_t* counts, silent_stream stream) try {
    NEED_CTX(ctx);
    return rgb_keypoints_dev<uint16_t>(ctx, "silent_rgb_keypoints_h", pyr, levels, n_levels, n_frames, p, top_percent, regions, orient_out,
                                       line_end_out, value_out, peak_value_out, idx, cap_per_frame, counts, stream);
} catch (...) {
    return on_exception(ctx, "silent_rgb_keypoints_h_dev");
}

// ------------------------------------------------------------------------------------------ gray pass + keypoints

// The gray pass (silent_gray_pass_dev, same maps bit for bit) with the keypoint epilogue in every kernel that writes `end`
// (silent_gray.h, GrayKp): value = value_from_color(pad_inwards(end, pad)) is folded into the per-level extrema, the value summary
// of the sparse tail and the NaN flags, or written as a map -- the end map is never read back for a reduction.  selection = 1:
// a-10 -> a-9 -> a-8 -> a-11 on (pad_inwards(end), value) with K channels, sparse like silent_rgb_keypoints (SILENT_TUNE_GRAY bit 6:
// the dense kernels for every level); selection = 0: a-11 on the value map (recognition_testing.py:90).
// The 16 arguments every silent_gray_keypoints* entry point has between n_frames and the stream, packed once at the ABI boundary
struct GrayKpArgs {
    const float *cs_kernel, *end_bank;
    int n_orient;
    float clip_hi, *pyr, *cs_out, *end_out;
    int pad, selection;
    double top_percent;
    const silent_extent* regions;
    float *value_out, *peak_value_out;
    int64_t* idx;
    size_t cap_per_frame;
    int64_t* counts;
};
#define KP_ARGS                                                                                                                           \
    const float *cs_kernel, const float *end_bank, int n_orient, float clip_hi, float *pyr, float *cs_out, float *end_out, int pad,       \
        int selection, double top_percent, const silent_extent *regions, float *value_out, float *peak_value_out, int64_t *idx,           \
        size_t cap_per_frame, int64_t *counts
#define KP_PACK \
    GrayKpArgs { cs_kernel, end_bank, n_orient, clip_hi, pyr, cs_out, end_out, pad, selection, top_percent, regions, value_out, peak_value_out, idx, cap_per_frame, counts }

// (everything the *_dev form refuses, before a launch and, in the host forms, before the batch is staged.)  FT: the frame element type
// -- float, uint8_t (silent_gray_keypoints_u8[_dev]) or FrameRgb8 (silent_gray_keypoints_u8x3[_dev]) -- of the ENTRY POINT (the view
// entry points check as a strided kind whatever kind then reads the view); has_frames: that argument is not NULL; maps_optional: pyr and
// end_out may be NULL (the host forms need neither map from the caller)
template <typename FT>
static int gray_keypoints_checks(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, bool has_frames, int n_frames,
                                 const GrayKpArgs& a, bool maps_optional) {
    const bool has_pyr = maps_optional || a.pyr, has_end = maps_optional || a.end_out;
    if (!plan || !has_frames || !has_pyr || !a.cs_kernel || !a.end_bank || !has_end || !a.regions || !a.counts || (!a.idx && a.cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (plan->ctx != ctx) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": plan belongs to another context");
    if constexpr (kFrameNarrow<FT>) TRY(check_narrow_frames<FT>(ctx, who, plan));
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": the plan must be single-channel");
    if (a.n_orient != 3 && a.n_orient != 4 && a.n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": n_orient must be 3, 4 or 8");
    if (n_frames < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": n_frames must be >= 1");
    if (a.pad < 0) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": pad must be >= 0");
    if (a.selection != 0 && a.selection != 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": selection must be 0 or 1");
    if (!a.selection && a.peak_value_out)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": peak_value_out needs selection = 1 (there is no peak-value map without it)");
    return SILENT_OK;
}

template <typename FT>
static int gray_keypoints_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, const GrayKpArgs& a,
                              silent_stream stream) {
    const char* who = entry_name<FT>(kGrayKeypoints);
    TRY(gray_keypoints_checks<FT>(ctx, who, plan, frames != nullptr, n_frames, a, false));
    hipStream_t s = (hipStream_t)stream;
    const silent_extent* levels = plan->extents.data();
    const int n_levels = plan->tab.n_levels;
    GrayKp kp;
    std::memset(&kp, 0, sizeof(kp));
    kp.n_levels = n_levels;
    kp.pad = a.pad;
    ctx->sparse_ran = false;
    if (!a.selection) {
        // a-11 straight on the value map: the epilogue writes it (into the head of the workspace unless the caller takes it)
        const size_t map_bytes = a.value_out ? 0 : align_up((size_t)plan->tab.frame_px_out * n_frames * sizeof(float));
        RegionPlan rp;
        TRY(region_prepare(ctx, who, levels, n_levels, n_frames, a.regions, map_bytes, s, &rp));
        kp.value_out = a.value_out ? a.value_out : (float*)ctx->ws.p;
        TRY(gray_pass_kp(ctx, plan, frames, n_frames, a.cs_kernel, a.end_bank, a.n_orient, a.clip_hi, a.pyr, a.cs_out, a.end_out, kp, s));
        return region_run(ctx, who, kp.value_out, levels, n_levels, n_frames, rp, a.idx, a.cap_per_frame, a.counts, s);
    }
    // The summary groups are kSumRows rows of a tile row; one SumTab geometry serves all levels, so both filter kernels must tile
    // with the same height (they do unless a build overrides SILENT_FUSED_TH; then the tail runs dense)
    const bool want_sparse = kFusedTH == kGrayTH && !(ctx->tune[SILENT_TUNE_GRAY] & 64u);
    SelectPlan sp;
    TRY(select_prepare(ctx, who, levels, n_levels, n_frames, a.regions, s, &sp, want_sparse ? kGrayTH : 0, !a.peak_value_out));
    const bool sparse = want_sparse && sp.st.frame_entries > 0;
    kp.mm = sp.mm;
    kp.nan_flags = sp.w.nan_flags;
    kp.value_out = a.value_out;
    if (sparse) {
        kp.sum = sp.w.sum;
        kp.sum_frame = sp.st.frame_entries;
        kp.gpt = sp.st.gpt;
        for (int l = 0; l < n_levels; ++l) kp.sum_off[l] = sp.st.off[l];
    }
    TRY(gray_pass_kp(ctx, plan, frames, n_frames, a.cs_kernel, a.end_bank, a.n_orient, a.clip_hi, a.pyr, a.cs_out, a.end_out, kp, s));
    publish_sparse_tail(ctx, sp, s, n_frames, n_levels, sparse);
    return select_run(ctx, who, a.end_out, nullptr, levels, n_levels, n_frames, a.n_orient, a.top_percent, sp, true, a.peak_value_out, a.idx,
                      a.cap_per_frame, a.counts, s, sparse, a.pad);
}

SILENT_EXPORT int silent_gray_keypoints_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames, KP_ARGS, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_keypoints_dev(ctx, plan, frames, n_frames, KP_PACK, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_dev");
}

// uint8 frames, read as they are (silent_hip.h): every output is silent_gray_keypoints_dev's on the widened frames
SILENT_EXPORT int silent_gray_keypoints_u8_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, KP_ARGS, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_keypoints_dev(ctx, plan, frames, n_frames, KP_PACK, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_u8_dev");
}

// interleaved 3-channel uint8 frames [n, H, W, 3], read as they are (silent_hip.h): every output is silent_gray_keypoints_dev's on
// the frame of values (b0 + b1 + b2) * float32(1/3)
SILENT_EXPORT int silent_gray_keypoints_u8x3_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, KP_ARGS, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_keypoints_dev(ctx, plan, rgb8(frames), n_frames, KP_PACK, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_u8x3_dev");
}

SILENT_EXPORT int silent_sparse_tail_stats(silent_ctx* ctx, int64_t* stats) try {
    NEED_CTX(ctx);
    if (!stats) return fail(ctx, SILENT_E_INVALID, "silent_sparse_tail_stats: stats is NULL");
    stats[0] = ctx->sparse_ran ? 1 : 0;
    stats[1] = stats[2] = stats[3] = stats[4] = 0;
    if (!ctx->sparse_ran || !ctx->ws.p) return SILENT_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->sparse_stream));
    std::vector<int> flags((size_t)ctx->sparse_pairs), cn((size_t)ctx->sparse_frames);
    HIP_TRY(ctx, hipMemcpy(flags.data(), (char*)ctx->ws.p + ctx->sparse_flags_off, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cn.data(), (char*)ctx->ws.p + ctx->sparse_candn_off, cn.size() * sizeof(int), hipMemcpyDeviceToHost));
    stats[1] = ctx->sparse_pairs;
    for (int f : flags) stats[2] += f == kTailDense ? 1 : 0;
    for (int f : flags) stats[4] += f == kTailZero ? 1 : 0;
    for (int c : cn) stats[3] += c;
    return SILENT_OK;
} catch (...) {
    return on_exception(ctx, "silent_sparse_tail_stats");
}

// ------------------------------------------------------------------------------------------ host-pointer twins

// some frame holds more keypoints than the caller's index buffer takes (the host forms report it: SILENT_E_CAPACITY)
static bool over_capacity(const int64_t* counts, int n_frames, size_t cap_per_frame) {
    return std::any_of(counts, counts + n_frames, [&](int64_t c) { return c > (int64_t)cap_per_frame; });
}

SILENT_EXPORT int silent_pad_inwards(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                     int n_frames, int channels, int pt, int pb, int pl, int pr, float* out) try {
    NEED_CTX(ctx);
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, "silent_pad_inwards: NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, "silent_pad_inwards: channels must be >= 1");
    long long px;
    TRY(check_levels(ctx, "silent_pad_inwards", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t b = (size_t)px * channels * 4;
    const int x = hs.in(in, b), o = hs.out(out, b);
    return hs.run([&] {
        return silent_pad_inwards_dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, channels, pt, pb, pl, pr, hs.dev<float>(o),
                                      nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_pad_inwards");
}

static int from_color_host(silent_ctx* ctx, const char* who,
                           int (*dev)(silent_ctx*, const float*, const silent_extent*, int, int, int, float*, silent_stream), const float* in,
                           const silent_extent* levels, int n_levels, int n_frames, int channels, float* out) {
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": channels must be >= 1");
    long long px;
    TRY(check_levels(ctx, who, levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const int x = hs.in(in, (size_t)px * channels * 4), o = hs.out(out, (size_t)px * 4);
    return hs.run([&] { return dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, channels, hs.dev<float>(o), nullptr); });
}

SILENT_EXPORT int silent_value_from_color(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                          int n_frames, int channels, float* out) try {
    NEED_CTX(ctx);
    return from_color_host(ctx, "silent_value_from_color", silent_value_from_color_dev, in, levels, n_levels, n_frames, channels, out);
} catch (...) {
    return on_exception(ctx, "silent_value_from_color");
}

SILENT_EXPORT int silent_bw_from_color(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                          int n_frames, int channels, float* out) try {
    NEED_CTX(ctx);
    return from_color_host(ctx, "silent_bw_from_color", silent_bw_from_color_dev, in, levels, n_levels, n_frames, channels, out);
} catch (...) {
    return on_exception(ctx, "silent_bw_from_color");
}

SILENT_EXPORT int silent_nms3x3(silent_ctx* ctx, const float* in, const silent_extent* levels, int n_levels,
                                int n_frames, int channels, int mode, float* out) try {
    NEED_CTX(ctx);
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, "silent_nms3x3: NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, "silent_nms3x3: channels must be >= 1");
    long long px;
    TRY(check_levels(ctx, "silent_nms3x3", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t b = (size_t)px * channels * 4;
    const int x = hs.in(in, b), o = hs.out(out, b);
    return hs.run([&] {
        return silent_nms3x3_dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, channels, mode, hs.dev<float>(o), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_nms3x3");
}

SILENT_EXPORT int silent_top_value_points(silent_ctx* ctx, const float* color, const float* value,
                                          const silent_extent* levels, int n_levels, int n_frames, int channels,
                                          double top_percent, float* out) try {
    NEED_CTX(ctx);
    if (!color || !out) return fail(ctx, SILENT_E_INVALID, "silent_top_value_points: NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, "silent_top_value_points: channels must be >= 1");
    long long px;
    TRY(check_levels(ctx, "silent_top_value_points", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t bc = (size_t)px * channels * 4;
    const int c = hs.in(color, bc), v = hs.in(value, (size_t)px * 4), o = hs.out(out, bc);
    return hs.run([&] {
        return silent_top_value_points_dev(ctx, hs.dev<float>(c), hs.dev<float>(v), levels, n_levels, n_frames, channels, top_percent,
                                           hs.dev<float>(o), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_top_value_points");
}

SILENT_EXPORT int silent_max_value_indices_region(silent_ctx* ctx, const float* value, const silent_extent* levels,
                                                  int n_levels, int n_frames, const silent_extent* regions,
                                                  int64_t* idx, size_t cap_per_frame, int64_t* counts) try {
    NEED_CTX(ctx);
    if (!value || !counts) return fail(ctx, SILENT_E_INVALID, "silent_max_value_indices_region: NULL pointer");
    long long px;
    TRY(check_levels(ctx, "silent_max_value_indices_region", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    // idx: only the first min(count, cap) rows of each frame are copied back, below
    const int v = hs.in(value, (size_t)px * 4), i = hs.scratch((size_t)n_frames * cap_per_frame * 4 * sizeof(int64_t)),
              c = hs.out(counts, (size_t)n_frames * sizeof(int64_t));
    TRY(hs.run([&] {
        return silent_max_value_indices_region_dev(ctx, hs.dev<float>(v), levels, n_levels, n_frames, regions, hs.dev<int64_t>(i),
                                                   cap_per_frame, hs.dev<int64_t>(c), nullptr);
    }));
    for (int f = 0; f < n_frames; ++f) {
        const size_t n = (size_t)std::min<int64_t>(counts[f], (int64_t)cap_per_frame), row = (size_t)f * cap_per_frame * 4;
        if (n) HIP_TRY(ctx, hipMemcpy(idx + row, hs.dev<int64_t>(i) + row, n * 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    if (over_capacity(counts, n_frames, cap_per_frame)) return fail(ctx, SILENT_E_CAPACITY, "silent_max_value_indices_region: cap_per_frame too small; counts hold the need");
    return SILENT_OK;
} catch (...) {
    return on_exception(ctx, "silent_max_value_indices_region");
}

SILENT_EXPORT int silent_rgb_keypoints(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                                       int n_frames, const silent_rgb_chain_params* p, double top_percent,
                                       const silent_extent* regions, float* orient_out, float* line_end_out, float* value_out,
                                       float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts) try {
    NEED_CTX(ctx);
    if (!pyr || !p || !regions || !counts || (!idx && cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, "silent_rgb_keypoints: NULL pointer");
    long long px;
    TRY(check_levels(ctx, "silent_rgb_keypoints", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t b1 = (size_t)px * 4, b3 = b1 * 3;
    // the *_dev form always needs the line-end map (the keypoints are taken from it)
    const int x = hs.in(pyr, b3), o = hs.out(orient_out, b3), l = line_end_out ? hs.out(line_end_out, b3) : hs.scratch(b3),
              v = hs.out(value_out, b1), pv = hs.out(peak_value_out, b1),
              i = hs.out(idx, (size_t)n_frames * cap_per_frame * 4 * sizeof(int64_t)),
              n = hs.out(counts, (size_t)n_frames * sizeof(int64_t));
    TRY(hs.run([&] {
        return silent_rgb_keypoints_dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, p, top_percent, regions, hs.dev<float>(o),
                                        hs.dev<float>(l), hs.dev<float>(v), hs.dev<float>(pv), hs.dev<int64_t>(i), cap_per_frame,
                                        hs.dev<int64_t>(n), nullptr);
    }));
    // idx / counts as silent_max_value_indices_region: the host form reports an index buffer that was too small
    if (over_capacity(counts, n_frames, cap_per_frame)) return fail(ctx, SILENT_E_CAPACITY, "silent_rgb_keypoints: cap_per_frame too small; counts hold the need");
    return SILENT_OK;
} catch (...) {
    return on_exception(ctx, "silent_rgb_keypoints");
}

SILENT_EXPORT int silent_rgb_keypoints_h(silent_ctx* ctx, const float* pyr, const silent_extent* levels, int n_levels,
                                         int n_frames, const silent_rgb_chain_params* p, double top_percent,
                                         const silent_extent* regions, uint16_t* orient_out, uint16_t* line_end_out, float* value_out,
                                         float* peak_value_out, int64_t* idx, size_t cap_per_frame, int64_t* counts) try {
    NEED_CTX(ctx);
    if (!pyr || !p || !regions || !line_end_out || !counts || (!idx && cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, "silent_rgb_keypoints_h: NULL pointer");
    long long px;
    TRY(check_levels(ctx, "silent_rgb_keypoints_h", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t b1 = (size_t)px * 4, b3 = (size_t)px * 3 * sizeof(uint16_t);
    const int x = hs.in(pyr, b1 * 3), o = hs.out(orient_out, b3), l = hs.out(line_end_out, b3), v = hs.out(value_out, b1),
              pv = hs.out(peak_value_out, b1), i = hs.out(idx, (size_t)n_frames * cap_per_frame * 4 * sizeof(int64_t)),
              n = hs.out(counts, (size_t)n_frames * sizeof(int64_t));
    TRY(hs.run([&] {
        return silent_rgb_keypoints_h_dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, p, top_percent, regions, hs.dev<uint16_t>(o),
                                          hs.dev<uint16_t>(l), hs.dev<float>(v), hs.dev<float>(pv), hs.dev<int64_t>(i), cap_per_frame,
                                          hs.dev<int64_t>(n), nullptr);
    }));
    if (over_capacity(counts, n_frames, cap_per_frame)) return fail(ctx, SILENT_E_CAPACITY, "silent_rgb_keypoints_h: cap_per_frame too small; counts hold the need");
    return SILENT_OK;
} catch (...) {
    return on_exception(ctx, "silent_rgb_keypoints_h");
}

// the host-pointer forms of silent_gray_keypoints on any frame type: the frames are staged as they are (frame_px_bytes each pixel)
template <typename FT>
static int gray_keypoints_host(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, const GrayKpArgs& a) {
    const char* who = entry_name<FT>(kGrayKeypoints);
    // (the host form accepts NULL pyr / end_out: the *_dev form needs both maps, they then live in the staging arena)
    TRY(gray_keypoints_checks<FT>(ctx, who, plan, frames != nullptr, n_frames, a, true));
    HostStage hs(ctx);
    const size_t b1 = (size_t)plan->tab.frame_px_out * n_frames * 4;
    const int x = hs.in(frames_host(frames), frames_bytes(plan, frames, n_frames)),
              p = a.pyr ? hs.out(a.pyr, b1) : hs.scratch(b1), cs = hs.out(a.cs_out, b1),
              end = a.end_out ? hs.out(a.end_out, b1 * a.n_orient) : hs.scratch(b1 * a.n_orient), v = hs.out(a.value_out, b1),
              pv = hs.out(a.peak_value_out, b1), i = hs.out(a.idx, (size_t)n_frames * a.cap_per_frame * 4 * sizeof(int64_t)),
              n = hs.out(a.counts, (size_t)n_frames * sizeof(int64_t));
    TRY(hs.run([&] {
        const StagedFrames<FT> staged(frames, hs.dev<char>(x));
        GrayKpArgs d = a;   // the same call on the staged buffers (pyr / end_out: the arena's, where the caller has none)
        d.pyr = hs.dev<float>(p), d.cs_out = hs.dev<float>(cs), d.end_out = hs.dev<float>(end);
        d.value_out = hs.dev<float>(v), d.peak_value_out = hs.dev<float>(pv), d.idx = hs.dev<int64_t>(i), d.counts = hs.dev<int64_t>(n);
        return gray_keypoints_dev(ctx, plan, staged.p, n_frames, d, nullptr);
    }));
    if (over_capacity(a.counts, n_frames, a.cap_per_frame)) return fail(ctx, SILENT_E_CAPACITY, std::string(who) + ": cap_per_frame too small; counts hold the need");
    return SILENT_OK;
}

SILENT_EXPORT int silent_gray_keypoints(silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n_frames, KP_ARGS) try {
    NEED_CTX(ctx);
    return gray_keypoints_host(ctx, plan, frames, n_frames, KP_PACK);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints");
}

SILENT_EXPORT int silent_gray_keypoints_u8(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, KP_ARGS) try {
    NEED_CTX(ctx);
    return gray_keypoints_host(ctx, plan, frames, n_frames, KP_PACK);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_u8");
}

SILENT_EXPORT int silent_gray_keypoints_u8x3(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint8_t* frames, int n_frames, KP_ARGS) try {
    NEED_CTX(ctx);
    return gray_keypoints_host(ctx, plan, rgb8(frames), n_frames, KP_PACK);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_u8x3");
}

// Strided uint8 views (silent_hip.h): the view's own refusals and those of the *_u8 form under the view's name, then the frame kind
// that reads it (with_view: a packed view takes the packed kernels).
static int gray_keypoints_view(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const silent_frame_view* view, int n_frames,
                               const GrayKpArgs& a, silent_stream stream) {
    const char* who = "silent_gray_keypoints_view";
    TRY(check_view(ctx, who, plan, view, n_frames, nullptr));
    // (the host form accepts NULL pyr / end_out, see gray_keypoints_host)
    TRY(gray_keypoints_checks<View8>(ctx, who, plan, true, n_frames, a, host));
    return with_view(plan, view, n_frames, [&](auto frames) {
        if (host) return gray_keypoints_host(ctx, plan, frames, n_frames, a);
        return gray_keypoints_dev(ctx, plan, frames, n_frames, a, stream);
    });
}

SILENT_EXPORT int silent_gray_keypoints_view_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                                 KP_ARGS, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_keypoints_view(ctx, false, plan, frames, n_frames, KP_PACK, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_view_dev");
}

SILENT_EXPORT int silent_gray_keypoints_view(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view* frames, int n_frames,
                                             KP_ARGS) try {
    NEED_CTX(ctx);
    return gray_keypoints_view(ctx, true, plan, frames, n_frames, KP_PACK, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_view");
}

// uint16 frames (silent_hip.h): the *_u8 forms with an unsigned 16-bit element, 2-byte aligned; strided uint16 views as the *_view forms
SILENT_EXPORT int silent_gray_keypoints_u16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames, KP_ARGS, silent_stream stream) try {
    NEED_CTX(ctx);
    TRY(check_u16_aligned(ctx, "silent_gray_keypoints_u16", frames));
    return gray_keypoints_dev(ctx, plan, frames, n_frames, KP_PACK, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_u16_dev");
}

SILENT_EXPORT int silent_gray_keypoints_u16(silent_ctx* ctx, const silent_pyramid_plan* plan, const uint16_t* frames, int n_frames, KP_ARGS) try {
    NEED_CTX(ctx);
    TRY(check_u16_aligned(ctx, "silent_gray_keypoints_u16", frames));
    return gray_keypoints_host(ctx, plan, frames, n_frames, KP_PACK);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_u16");
}

static int gray_keypoints_view16(silent_ctx* ctx, bool host, const silent_pyramid_plan* plan, const silent_frame_view16* view, int n_frames,
                                 const GrayKpArgs& a, silent_stream stream) {
    const char* who = "silent_gray_keypoints_view16";
    TRY(check_view16(ctx, who, plan, view, n_frames, nullptr));
    // (the host form accepts NULL pyr / end_out, see gray_keypoints_host)
    TRY(gray_keypoints_checks<View16>(ctx, who, plan, true, n_frames, a, host));
    return with_view16(plan, view, n_frames, [&](auto frames) {
        if (host) return gray_keypoints_host(ctx, plan, frames, n_frames, a);
        return gray_keypoints_dev(ctx, plan, frames, n_frames, a, stream);
    });
}

SILENT_EXPORT int silent_gray_keypoints_view16_dev(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                                   KP_ARGS, silent_stream stream) try {
    NEED_CTX(ctx);
    return gray_keypoints_view16(ctx, false, plan, frames, n_frames, KP_PACK, stream);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_view16_dev");
}

SILENT_EXPORT int silent_gray_keypoints_view16(silent_ctx* ctx, const silent_pyramid_plan* plan, const silent_frame_view16* frames, int n_frames,
                                               KP_ARGS) try {
    NEED_CTX(ctx);
    return gray_keypoints_view16(ctx, true, plan, frames, n_frames, KP_PACK, nullptr);
} catch (...) {
    return on_exception(ctx, "silent_gray_keypoints_view16");
}
#undef KP_ARGS
#undef KP_PACK

SILENT_EXPORT int silent_centroids(silent_ctx* ctx, const float* value, const silent_extent* levels, int n_levels,
                                   int n_frames, int region_h, int region_w, float* dist_out, float* total_out) try {
    NEED_CTX(ctx);
    if (!value || !dist_out || !total_out) return fail(ctx, SILENT_E_INVALID, "silent_centroids: NULL pointer");
    long long px;
    TRY(check_levels(ctx, "silent_centroids", levels, n_levels, n_frames, &px));
    CellTab ct;
    TRY(refuse(ctx, "silent_centroids", build_cell_tab(levels, n_levels, region_h, region_w, &ct)));
    HostStage hs(ctx);
    const int v = hs.in(value, (size_t)px * 4), d = hs.out(dist_out, (size_t)px * 4),
              t = hs.out(total_out, (size_t)ct.frame_cells * n_frames * 4);
    return hs.run([&] {
        return silent_centroids_dev(ctx, hs.dev<float>(v), levels, n_levels, n_frames, region_h, region_w, hs.dev<float>(d),
                                    hs.dev<float>(t), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_centroids");
}

SILENT_EXPORT int silent_boosting_step(silent_ctx* ctx, const float* input, const silent_extent* levels, int n_levels,
                                       int n_frames, const silent_boosting_params* params, float* energy,
                                       float* fired_out, float* energy_out) try {
    NEED_CTX(ctx);
    if (!input || !energy || !fired_out) return fail(ctx, SILENT_E_INVALID, "silent_boosting_step: NULL pointer");
    BoostP bp;
    TRY(refuse(ctx, "silent_boosting_step", boost_params(params, &bp)));
    long long px;
    TRY(check_levels(ctx, "silent_boosting_step", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t b1 = (size_t)px * 4, bc = b1 * (bp.visualize ? 3 : 1);
    const int x = hs.in(input, b1), e = hs.inout(energy, b1), f = hs.out(fired_out, bc), o = hs.out(energy_out, bc);
    return hs.run([&] {
        return silent_boosting_step_dev(ctx, hs.dev<float>(x), levels, n_levels, n_frames, params, hs.dev<float>(e), hs.dev<float>(f),
                                        hs.dev<float>(o), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_boosting_step");
}

SILENT_EXPORT int silent_affine_clip(silent_ctx* ctx, const float* in, size_t n_values,
                                     const silent_affine_params* params, float* out) try {
    NEED_CTX(ctx);
    if (!in || !out || !params) return fail(ctx, SILENT_E_INVALID, "silent_affine_clip: NULL pointer");
    if (n_values == 0) return fail(ctx, SILENT_E_INVALID, "silent_affine_clip: empty tensor");
    HostStage hs(ctx);
    const int x = hs.in(in, n_values * 4), o = hs.out(out, n_values * 4);
    return hs.run([&] { return silent_affine_clip_dev(ctx, hs.dev<float>(x), n_values, params, hs.dev<float>(o), nullptr); });
} catch (...) {
    return on_exception(ctx, "silent_affine_clip");
}

SILENT_EXPORT int silent_cast_interleave(silent_ctx* ctx, const void* in, int in_dtype, size_t n_pixels, int in_stride,
                                         int in_offset, int count, float* out, int out_stride, int out_offset) try {
    NEED_CTX(ctx);
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, "silent_cast_interleave: NULL pointer");
    const size_t es = dtype_size(in_dtype);
    if (!es) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_cast_interleave: unknown in_dtype");
    if (n_pixels == 0 || in_stride < 1 || out_stride < 1) return fail(ctx, SILENT_E_INVALID, "silent_cast_interleave: empty tensor");
    if (count < 1 || in_offset < 0 || out_offset < 0 || in_stride < in_offset + count || out_stride < out_offset + count)
        return fail(ctx, SILENT_E_INVALID, "silent_cast_interleave: need 0 <= offset and offset + count <= stride on both sides");
    HostStage hs(ctx);
    // the last pixel needs offset + count elements, not a whole stride: a caller's buffer may end with its last used element
    const int x = hs.in(in, ((n_pixels - 1) * (size_t)in_stride + (size_t)(in_offset + count)) * es);
    // in / out: the elements of out that this call does not write keep their values
    const int o = hs.inout(out, ((n_pixels - 1) * (size_t)out_stride + (size_t)(out_offset + count)) * 4);
    return hs.run([&] {
        return silent_cast_interleave_dev(ctx, hs.dev<char>(x), in_dtype, n_pixels, in_stride, in_offset, count, hs.dev<float>(o),
                                          out_stride, out_offset, nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_cast_interleave");
}

SILENT_EXPORT int silent_resize_nearest(silent_ctx* ctx, const float* in, const silent_extent* in_levels, int n_levels,
                                        int n_frames, int channels, const silent_extent* out_levels, float* out) try {
    NEED_CTX(ctx);
    if (!in || !out) return fail(ctx, SILENT_E_INVALID, "silent_resize_nearest: NULL pointer");
    if (channels < 1) return fail(ctx, SILENT_E_INVALID, "silent_resize_nearest: channels must be >= 1");
    long long ipx, opx;
    TRY(check_levels(ctx, "silent_resize_nearest", in_levels, n_levels, n_frames, &ipx));
    TRY(check_levels(ctx, "silent_resize_nearest", out_levels, n_levels, n_frames, &opx));
    HostStage hs(ctx);
    const int x = hs.in(in, (size_t)ipx * channels * 4), o = hs.out(out, (size_t)opx * channels * 4);
    return hs.run([&] {
        return silent_resize_nearest_dev(ctx, hs.dev<float>(x), in_levels, n_levels, n_frames, channels, out_levels, hs.dev<float>(o),
                                         nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_resize_nearest");
}

SILENT_EXPORT int silent_select_peaks(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                                      int n_levels, int n_frames, int channels, double top_percent, float* top_out,
                                      float* peaks_out, float* peak_value_out) try {
    NEED_CTX(ctx);
    if (!color) return fail(ctx, SILENT_E_INVALID, "silent_select_peaks: NULL pointer");
    if (!top_out && !peaks_out && !peak_value_out) return fail(ctx, SILENT_E_INVALID, "silent_select_peaks: all outputs are NULL");
    if (!select_channels_ok(channels)) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_select_peaks: channels must be 1, 3, 4 or 8");
    long long px;
    TRY(check_levels(ctx, "silent_select_peaks", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t bc = (size_t)px * channels * 4, bv = (size_t)px * 4;
    const int c = hs.in(color, bc), v = hs.in(value, bv), t = hs.out(top_out, bc), pk = hs.out(peaks_out, bc),
              pv = hs.out(peak_value_out, bv);
    return hs.run([&] {
        return silent_select_peaks_dev(ctx, hs.dev<float>(c), hs.dev<float>(v), levels, n_levels, n_frames, channels, top_percent,
                                       hs.dev<float>(t), hs.dev<float>(pk), hs.dev<float>(pv), nullptr);
    });
} catch (...) {
    return on_exception(ctx, "silent_select_peaks");
}

SILENT_EXPORT int silent_select_keypoints(silent_ctx* ctx, const float* color, const float* value, const silent_extent* levels,
                                          int n_levels, int n_frames, int channels, double top_percent,
                                          const silent_extent* regions, float* peak_value_out, int64_t* idx,
                                          size_t cap_per_frame, int64_t* counts) try {
    NEED_CTX(ctx);
    if (!color || !regions || !counts || (!idx && cap_per_frame))
        return fail(ctx, SILENT_E_INVALID, "silent_select_keypoints: NULL pointer");
    if (!select_channels_ok(channels)) return fail(ctx, SILENT_E_UNSUPPORTED, "silent_select_keypoints: channels must be 1, 3, 4 or 8");
    long long px;
    TRY(check_levels(ctx, "silent_select_keypoints", levels, n_levels, n_frames, &px));
    HostStage hs(ctx);
    const size_t bv = (size_t)px * 4;
    const int c = hs.in(color, bv * channels), v = hs.in(value, bv), pv = hs.out(peak_value_out, bv),
              i = hs.out(idx, (size_t)n_frames * cap_per_frame * 4 * sizeof(int64_t)),
              n = hs.out(counts, (size_t)n_frames * sizeof(int64_t));
    TRY(hs.run([&] {
        return silent_select_keypoints_dev(ctx, hs.dev<float>(c), hs.dev<float>(v), levels, n_levels, n_frames, channels, top_percent,
                                           regions, hs.dev<float>(pv), hs.dev<int64_t>(i), cap_per_frame, hs.dev<int64_t>(n), nullptr);
    }));
    // idx / counts as silent_max_value_indices_region: the host form reports an index buffer that was too small
    if (over_capacity(counts, n_frames, cap_per_frame)) return fail(ctx, SILENT_E_CAPACITY, "silent_select_keypoints: cap_per_frame too small; counts hold the need");
    return SILENT_OK;
} catch (...) {
    return on_exception(ctx, "silent_select_keypoints");
}
