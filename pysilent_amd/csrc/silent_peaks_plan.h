// The host planning of the keypoint tail (a-10 -> a-9 -> a-8 -> a-11), the centroids and the boosting state (silent_peaks_api.hip) as
// plain functions over plain structs.  Nothing here makes a HIP call or sees the context: a refusal comes back as a status and the tail
// of its message, and the entry point reports it under its own name.  What these build is pinned line for line by
// tests/golden/kp_tables.txt (tests/kp_tables_host_main.cpp prints it, tests/test_kp_tables_host.py).
#pragma once
#include "silent_peaks.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace silent {
struct Refusal {
    int status = SILENT_OK;
    const char* tail = "";   // what follows the entry point's name in the message
};

// ------------------------------------------------------------------------------------------ a-11: region tables
// TF1 max_pool SAME geometry with window == full extent
inline int region_axis(int size, int stride, int* n_win, int* nseg, int* cut, int* w_lo, int* w_hi, float* scale) {
    if (stride < 1) return -1;
    const int out = (size + stride - 1) / stride;
    *n_win = out;
    *scale = (float)out / (float)size;
    if (out > kMaxWin) return -2;
    const int pad_before = ((out - 1) * stride) / 2;
    int lo[kMaxWin], hi[kMaxWin];
    std::vector<int> cuts = {0, size};
    for (int j = 0; j < out; ++j) {
        const int a = j * stride - pad_before, b = a + size;
        lo[j] = a < 0 ? 0 : a;
        hi[j] = b > size ? size : b;
        cuts.push_back(lo[j]);
        cuts.push_back(hi[j]);
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    const int ns = (int)cuts.size() - 1;
    if (ns > kMaxSeg) return -2;
    for (int i = 0; i <= ns; ++i) cut[i] = cuts[i];
    for (int j = 0; j < out; ++j) {
        int a = 0, b = 0;
        for (int i = 0; i <= ns; ++i) {
            if (cuts[i] == lo[j]) a = i;
            if (cuts[i] == hi[j]) b = i;
        }
        w_lo[j] = a;
        w_hi[j] = b;
    }
    *nseg = ns;
    return 0;
}

// Region tables of max_value_indices_region (TF1 max_pool geometry per level).  *general = true when some level has more
// than kMaxWin windows per axis: the cell tables (kernarg-resident) do not apply then and the separable prefix / suffix
// path runs (region_rowmax_kernel / region_colmax_kernel) -- any region_shape the reference accepts
// (slam_recognition/util/selection/top_value_points.py:32-45).
inline Refusal build_region_tab(const silent_extent* levels, int n_levels, const silent_extent* regions, RegionTab* rt, bool* general) {
    std::memset(rt, 0, sizeof(*rt));
    *general = false;
    long long m1 = 0, pooled = 0;
    for (int l = 0; l < n_levels; ++l) {
        RegionLevel& r = rt->lv[l];
        if (regions[l].h < 1 || regions[l].w < 1) return {SILENT_E_INVALID, ": region extents must be >= 1"};
        const int rc0 = region_axis(levels[l].h, regions[l].h, &r.oh, &r.nrs, r.rcut, r.wy_lo, r.wy_hi, &r.yscale);
        const int rc1 = region_axis(levels[l].w, regions[l].w, &r.ow, &r.ncs, r.ccut, r.wx_lo, r.wx_hi, &r.xscale);
        if (rc0 == -2 || rc1 == -2) *general = true;
        r.ry = regions[l].h;
        r.rx = regions[l].w;
        r.pad_y = ((r.oh - 1) * r.ry) / 2;
        r.pad_x = ((r.ow - 1) * r.rx) / 2;
        r.m1_off = m1;
        r.pooled_off = pooled;
        m1 += (long long)levels[l].h * r.ow;
        pooled += (long long)r.oh * r.ow;
    }
    rt->m1_per_frame = m1;
    rt->pooled_per_frame = pooled;
    return {};
}

// ------------------------------------------------------------------------------------------ sparse tail: value summary
// Geometry of the value summary a chain launch with tile height th leaves (silent_rgb2.h): per level
// [tiles_y * gpt][ceil(w / 2)] entries, gpt = ceil(th / kSumRows).  All zero -- frame_entries = 0, the tail runs dense -- where no
// summary is asked for (th <= 0) or the sparse kernels do not apply: the general region path, more frames than sparse_select_kernel's
// grid.y takes, or a frame of 2^31 entries (it indexes a frame with int)
inline void build_sum_tab(const silent_extent* levels, int n_levels, int n_frames, int th, bool general, SumTab* st) {
    std::memset(st, 0, sizeof(*st));
    if (th <= 0 || general || n_frames > 65535) return;
    st->th = th;
    st->gpt = (th + kSumRows - 1) / kSumRows;
    long long e = 0;
    for (int l = 0; l < n_levels; ++l) {
        st->off[l] = e;
        e += (long long)((levels[l].h + th - 1) / th) * st->gpt * ((levels[l].w + 1) / 2);
    }
    for (int l = n_levels; l <= kMaxLevels; ++l) st->off[l] = e;
    st->frame_entries = e;
    if (e >= (1ll << 31)) std::memset(st, 0, sizeof(*st));
}

// ------------------------------------------------------------------------------------------ keypoint workspace
// Byte offsets of the pieces of the keypoint passes' workspace, in workspace order
struct KeypointLayout {
    size_t cells, chunk_counts, hit_masks, cand_n, nan_flags, chunk_offsets, m1, pooled, sum, cand, dense_flags, pv;
    size_t n_cells, zero_from, zero_bytes, total;
};

// reserve: bytes the caller keeps for itself at the head; blocks: of the count / write passes (kKpChunk pixels each); sum_entries: the
// SumTab's frame_entries (0: no sparse tail -- `sum` and `cand` are empty); pv_px: pixels per frame of a peak-value map in the workspace.
// One bump pointer carves it: every piece starts 256-aligned (init_select_kernel zeroes with uint4 stores and relies on it); the zero
// range runs from the first piece marked `zeroed` to the end of the last, so those pieces are taken next to each other
// (tests/kp_tables_host_main.cpp checks that the range holds them and nothing else)
inline KeypointLayout keypoint_layout(int n_levels, int n_frames, long long blocks, size_t reserve, const RegionTab& rt, bool general,
                                      long long sum_entries, long long pv_px) {
    const size_t nf = (size_t)n_frames, pairs = nf * n_levels, nb = (size_t)blocks;
    size_t at = 0, zero_lo = ~(size_t)0, zero_hi = 0;
    auto take = [&](size_t bytes, bool zeroed = false) {
        const size_t off = at;
        at += (bytes + 255) / 256 * 256;
        if (zeroed) zero_lo = std::min(zero_lo, off), zero_hi = at;
        return off;
    };
    KeypointLayout k;
    k.n_cells = pairs * kCells;
    take(reserve);
    k.cells = take(k.n_cells * sizeof(unsigned));
    k.chunk_counts = take(nb * sizeof(int), true);
    k.hit_masks = take(nb * 4 * kKpPer * sizeof(unsigned long long), true);   // 1 bit per pixel
    k.cand_n = take(nf * sizeof(int), true);
    k.nan_flags = take(pairs * sizeof(int), true);
    k.chunk_offsets = take(nb * sizeof(long long));
    k.m1 = take(general ? nf * rt.m1_per_frame * sizeof(float) : 0);
    k.pooled = take(general ? nf * rt.pooled_per_frame * sizeof(float) : 0);
    k.sum = take((size_t)sum_entries * nf * sizeof(float));
    k.cand = take(sum_entries ? nf * kCandCap * sizeof(Candidate) : 0);
    k.dense_flags = take(pairs * sizeof(int));
    k.pv = take((size_t)pv_px * nf * sizeof(float));
    k.zero_from = zero_lo;
    k.zero_bytes = zero_hi - zero_lo;
    k.total = at;
    return k;
}

// ------------------------------------------------------------------------------------------ centroids
inline Refusal build_cell_tab(const silent_extent* levels, int n_levels, int rh, int rw, CellTab* ct) {
    if (rh < 1 || rw < 1) return {SILENT_E_INVALID, ": region extents must be >= 1"};
    std::memset(ct, 0, sizeof(*ct));
    ct->rh = rh;
    ct->rw = rw;
    long long cells = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int h = levels[l].h, w = levels[l].w;
        ct->oh[l] = (h + rh - 1) / rh;
        ct->ow[l] = (w + rw - 1) / rw;
        ct->y_first[l] = -(std::max((ct->oh[l] - 1) * rh + rh - h, 0) / 2);
        ct->x_first[l] = -(std::max((ct->ow[l] - 1) * rw + rw - w, 0) / 2);
        ct->yscale[l] = (float)ct->oh[l] / (float)h;
        ct->xscale[l] = (float)ct->ow[l] / (float)w;
        ct->cell_off[l] = cells;
        cells += (long long)ct->oh[l] * ct->ow[l];
    }
    ct->frame_cells = cells;
    return {};
}

// ------------------------------------------------------------------------------------------ boosting state
// (the messages are silent_boosting_step's, whoever asks)
inline Refusal boost_params(const silent_boosting_params* p, BoostP* bp) {
    if (!p) return {SILENT_E_INVALID, ": NULL params"};
    if (p->recovery_mode < 1 || p->recovery_mode > 3) return {SILENT_E_INVALID, ": You must choose a type of recovery"};
    bp->lo = -p->exhaustion_max;
    bp->hi = p->excitation_max;
    bp->recovery_mode = (int)p->recovery_mode;
    bp->recovery_amount = p->recovery_amount;
    bp->recovery_percentage = p->recovery_percentage;
    bp->visualize = p->visualize ? 1 : 0;
    const double span = (double)p->exhaustion_max + (double)p->excitation_max;
    bp->normer = (float)(255.0 / span);
    bp->centerer = (float)(((double)p->excitation_max / span) * 255.0);
    return {};
}

// ------------------------------------------------------------------------------------------ attention tail
// (silent_attention_tail: centroids at two scales + the boosting state on a packed pyramid, silent_peaks.h AttnTab)
// The geometry: per level the cells of the map, the extents of the nearest-neighbour half map -- (int)((float)h / resize_div), the
// float32 division and truncation of recognition_testing.py:82-83 -- and its cells
inline Refusal attention_extents(const silent_extent* levels, int n_levels, int rh, int rw, float resize_div, silent_extent* cells,
                                 silent_extent* half, silent_extent* cells2) {
    if (!levels) return {SILENT_E_INVALID, ": levels is NULL"};
    if (n_levels < 1 || n_levels > kMaxLevels) return {SILENT_E_INVALID, ": n_levels must be in [1, SILENT_MAX_LEVELS]"};
    if (rh < 1 || rw < 1) return {SILENT_E_INVALID, ": region extents must be >= 1"};
    if (!(resize_div >= 1.0f) || !(resize_div <= 3.402823466e+38f)) return {SILENT_E_INVALID, ": resize_div must be finite and >= 1"};
    for (int l = 0; l < n_levels; ++l) {
        const long long h = levels[l].h, w = levels[l].w;
        if (h < 1 || w < 1 || h * w > (1ll << 30)) return {SILENT_E_INVALID, ": a level extent is not positive (or above 2^30 pixels)"};
        const silent_extent hf = {(int)((float)levels[l].h / resize_div), (int)((float)levels[l].w / resize_div)};
        if (hf.h < 1 || hf.w < 1) return {SILENT_E_INVALID, ": a level is too small for a half extent (h or w below resize_div)"};
        if (cells) cells[l] = silent_extent{(levels[l].h + rh - 1) / rh, (levels[l].w + rw - 1) / rw};
        if (half) half[l] = hf;
        if (cells2) cells2[l] = silent_extent{(hf.h + rh - 1) / rh, (hf.w + rw - 1) / rw};
    }
    return {};
}

// The four affine steps of the tail (recognition_testing.py:79-81, :99), the same for its two forms: T is AttnTab or DispTail
template <class T>
inline void tail_affines(T* t) {
    t->by255 = AffineP{1.f, 255.f, 0.f, -INFINITY, INFINITY, 0.f};                  // value / 255
    t->imp = AffineP{255.f / 4.0f, 1.f, 0.f, 1.f, 256.f, -1.f};                     // clip(total * 255 / 4, 1, 256) - 1
    t->inv = AffineP{-255.f, 1.f, 255.f, -INFINITY, INFINITY, 0.f};                 // 255 - dist * 255
    t->x255 = AffineP{255.f, 1.f, 0.f, -INFINITY, INFINITY, 0.f};                   // fired * 255
}

// Byte offsets of the pieces of the tail's workspace, in workspace order: the centroids of both maps ([cells][2]), the importances
// and importances ** energy of the map's cells -- 8 + 8 + 4 + 4 bytes per cell, every piece 256-aligned
struct AttnLayout {
    size_t cxy, cxy2, imp, m, total;
};
inline AttnLayout attention_layout(long long cells, long long cells2) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t off = at;
        at += (bytes + 255) / 256 * 256;
        return off;
    };
    AttnLayout k;
    k.cxy = take((size_t)cells * 2 * sizeof(float));
    k.cxy2 = take((size_t)cells2 * 2 * sizeof(float));
    k.imp = take((size_t)cells * sizeof(float));
    k.m = take((size_t)cells * sizeof(float));
    k.total = at;
    return k;
}

// Everything the two launches need but the pointers: the tables (AttnTab, a kernel argument), block counts, cell totals, workspace.
// with_half = false (no centroids2_out): nothing of the half map is planned -- no cells, no blocks, no workspace.
struct AttnPlan {
    AttnTab t;
    silent_extent cells[kMaxLevels], half[kMaxLevels], cells2[kMaxLevels];
    long long n_cells, n_cells2;          // of all frames
    long long px_blocks, px2_blocks, cell_blocks;   // attn_pixels_kernel: tiles of the map, of the half map, chunks of the map's cells
    long long frame_px, frame_px2;
    AttnLayout ws;
};
inline Refusal attention_plan(const silent_extent* levels, int n_levels, int n_frames, const silent_attention_params* p, bool with_dist,
                              bool with_half, AttnPlan* ap) {
    if (!p) return {SILENT_E_INVALID, ": NULL params"};
    if (n_levels < 1 || n_levels > kMaxLevels) return {SILENT_E_INVALID, ": n_levels must be in [1, SILENT_MAX_LEVELS]"};
    if (n_frames < 1) return {SILENT_E_INVALID, ": n_frames must be >= 1"};
    Refusal r = attention_extents(levels, n_levels, p->region_h, p->region_w, p->resize_div, ap->cells, ap->half, ap->cells2);
    if (r.status != SILENT_OK) return r;
    AttnTab& t = ap->t;
    std::memset(&t, 0, sizeof(t));
    r = boost_params(&p->boosting, &t.bp);
    if (r.status != SILENT_OK) return r;
    (void)build_cell_tab(levels, n_levels, p->region_h, p->region_w, &t.ct1);       // (the region extents were checked above)
    (void)build_cell_tab(ap->half, n_levels, p->region_h, p->region_w, &t.ct2);
    for (int l = 0; l < n_levels; ++l) {
        t.yscale_r[l] = (float)levels[l].h / (float)ap->half[l].h;                  // (silent_resize_nearest: float32 in / out)
        t.xscale_r[l] = (float)levels[l].w / (float)ap->half[l].w;
    }
    // the three index spaces of attn_pixels_kernel: tiles of kAttnTW x kAttnTH pixels of both maps, chunks of kChunk cells
    ap->px_blocks = fill_level_tab(levels, n_levels, n_frames, kAttnTW, kAttnTH, nullptr, &t.tab1);
    ap->px2_blocks = fill_level_tab(ap->half, n_levels, n_frames, kAttnTW, kAttnTH, nullptr, &t.tab2);
    ap->cell_blocks = fill_level_tab(ap->cells, n_levels, n_frames, kChunk, 0, nullptr, &t.tabc);
    ap->frame_px = t.tab1.frame_px;
    ap->frame_px2 = t.tab2.frame_px;
    ap->n_cells = t.ct1.frame_cells * n_frames;
    ap->n_cells2 = with_half ? t.ct2.frame_cells * n_frames : 0;
    if (!with_dist) ap->px_blocks = 0;
    if (!with_half) ap->px2_blocks = 0;
    t.b1 = (unsigned)std::min<long long>(ap->px_blocks, 0x7fffffffll);
    t.b2 = (unsigned)std::min<long long>(ap->px_blocks + ap->px2_blocks, 0x7fffffffll);
    t.n_frames = n_frames;
    t.n_cells = ap->n_cells;
    t.n_cells2 = ap->n_cells2;
    if (ap->px_blocks + ap->px2_blocks + ap->cell_blocks > 0x7fffffffll || (ap->n_cells + ap->n_cells2 + 255) / 256 > 0x7fffffffll)
        return {SILENT_E_INVALID, ": too many tiles for one launch"};
    tail_affines(&t);
    ap->ws = attention_layout(ap->n_cells, ap->n_cells2);
    return {};
}

}  // namespace silent
