// The planner behind silent_pyramid_plan_create_ex (silent_pyramid_api.hip) as steps.  Nothing here makes a HIP call: every step fills
// host vectors and structs from the level geometry, the caller uploads them and wires the device pointers.  What the steps build is
// pinned byte for byte by tests/golden/plan_tables.txt (tests/plan_tables_host_main.cpp prints it, tests/test_plan_tables_host.py).
#pragma once
#include "silent_plan.h"

#include <limits>

namespace silent {
// ------------------------------------------------------------------------------------------ axis tables
inline void spline5_weights(double t, double* w) {
    // quintic cardinal B-spline at taps floor(c)-2 .. floor(c)+3; last tap by partition of unity
    const double y = t, z = 1.0 - t;
    double t2 = y * y;
    w[2] = t2 * (t2 * (0.25 - y / 12.0) - 0.5) + 0.55;
    t2 = z * z;
    w[3] = t2 * (t2 * (0.25 - z / 12.0) - 0.5) + 0.55;
    const double y1 = y + 1.0;
    w[1] = y1 * (y1 * (y1 * (y1 * (y1 / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
    const double z1 = z + 1.0;
    w[4] = z1 * (z1 * (z1 * (z1 * (z1 / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
    const double y2 = 1.0 - y;
    w[0] = y2 * y2 * y2 * y2 * y2 / 120.0;
    w[5] = 1.0 - w[0] - w[1] - w[2] - w[3] - w[4];
}
inline int host_mirror(long i, int n) {
    if (n == 1) return 0;
    const long period = 2L * (n - 1);
    if (i < 0) i = -i;
    i %= period;
    return (int)(i >= n ? period - i : i);
}
// scipy.ndimage.zoom, grid_mode=False: output o samples o * (n_in-1)/(n_out-1); mode 'constant'
// declares a coordinate outside [0, n_in-1] out of bounds (-> cval 0 for the whole row/column).
// wts64 (may be NULL): the same weights as scipy's float64 values (F64 plans)
inline void axis_table(int n_in, int n_out, int* base, int* idx, float* wts, double* wts64) {
    const double step = n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 1.0;
    for (int o = 0; o < n_out; ++o) {
        const double c = (double)o * step;
        const long b = (long)std::floor(c);
        double w[6] = {0, 0, 0, 0, 0, 0};
        if (c >= 0.0 && c <= (double)(n_in - 1)) spline5_weights(c - (double)b, w);
        base[o] = (int)b;
        for (int j = 0; j < 6; ++j) {
            // a weight that is not 0 in scipy's double arithmetic must not become 0 in float32: an outer tap's (1 - t)^5 / 120 falls
            // below 2^-149 when t rounds to just under 1, and 0 * inf = NaN where scipy has tiny * inf = inf.  The smallest float32
            // magnitude keeps the sign and the non-finite arithmetic; next to finite pixels it is as invisible as the true weight
            float f = (float)w[j];
            if (w[j] != 0.0 && f == 0.0f) f = std::copysign(std::numeric_limits<float>::denorm_min(), (float)(w[j] < 0.0 ? -1.0 : 1.0));
            wts[6 * o + j] = f;
            if (wts64) wts64[6 * o + j] = w[j];
            idx[6 * o + j] = host_mirror(b - 2 + j, n_in);
        }
    }
}

// The host tap tables of every level (entries xtab_off / ytab_off of PyrLevelDev, 6 taps each) and the region-start tables
struct AxisTables {
    std::vector<int> xbase, xidx, ybase, yidx, xreg, yreg;
    std::vector<float> xw, yw;
    std::vector<double> xw64, yw64;   // F64 plans
};
// One axis of a general level on regions of R pixels: outputs are owned by the region that holds their ANCHOR = floor(source
// coordinate), frame coordinates -- `regions` + 1 starts are appended to reg.  Every mirrored tap of an anchored output must lie inside
// its region's staged tile (see the kernel): false where one does not.
inline bool region_table(const int* base, const int* idx, int n_out, int src0, int regions, int R, int halo_lo, int halo_hi, std::vector<int>& reg) {
    int o = 0;
    for (int r = 0; r <= regions; ++r) {
        while (o < n_out && base[o] + src0 < r * R) ++o;
        reg.push_back(r == regions ? n_out : o);
    }
    bool ok = true;
    for (o = 0; o < n_out; ++o) {
        const int R0 = ((base[o] + src0) / R) * R;
        for (int j = 0; j < 6; ++j) {
            const int p = idx[(size_t)o * 6 + j] + src0 - (R0 - halo_lo);
            if (p < 0 || p >= R + halo_lo + halo_hi) ok = false;
        }
    }
    return ok;
}
// The frame and the levels as the kernels' records: geometry, offsets into the tap tables and into one pyramid, the canvases.  The
// index of the first level whose geometry is invalid, or -1.
inline int build_levels(PyrTab& tab, int frame_h, int frame_w, int channels, const silent_pyr_level* levels, int n_levels,
                        std::vector<silent_extent>& extents) {
    tab.n_levels = n_levels; tab.H = frame_h; tab.W = frame_w; tab.C = channels;
    tab.regions_x = (frame_w + region_w(channels) - 1) / region_w(channels);
    tab.regions_y = (frame_h + region_h(channels) - 1) / region_h(channels);
    long long cols = 0, rows = 0, px = 0;
    for (int l = 0; l < n_levels; ++l) {
        const silent_pyr_level& L = levels[l];
        const bool ok = L.src_h >= 1 && L.src_w >= 1 && L.src_y0 >= 0 && L.src_x0 >= 0 &&
                        (long long)L.src_y0 + L.src_h <= frame_h && (long long)L.src_x0 + L.src_w <= frame_w &&
                        L.zoom_h >= 1 && L.zoom_w >= 1 && L.out_h >= 1 && L.out_w >= 1 &&
                        (long long)L.out_h * L.out_w <= (1ll << 30) && (long long)L.zoom_h * L.zoom_w <= (1ll << 30);
        if (!ok) return l;
        PyrLevelDev& d = tab.lv[l];
        d.src_y0 = L.src_y0; d.src_x0 = L.src_x0; d.src_h = L.src_h; d.src_w = L.src_w;
        d.zoom_h = L.zoom_h; d.zoom_w = L.zoom_w; d.out_h = L.out_h; d.out_w = L.out_w;
        d.xtab_off = (int)cols;
        d.ytab_off = (int)rows;
        cols += L.zoom_w;
        rows += L.zoom_h;
        tab.px_off[l] = px;
        px += (long long)L.out_h * L.out_w;
        extents.push_back(silent_extent{L.out_h, L.out_w});
    }
    tab.frame_px_out = px;
    return -1;
}
// The scipy tap tables of every level (F64 plans: also as float64), its class -- unit or general --, the unit tiles and zero chunks of the
// launches, a general level's dead last row / column trimmed, its region tables.  unit_w / unit_w64: the six taps of a unit level.
inline bool build_axis_tables(PyrTab& tab, bool f64, AxisTables& ax, float* unit_w, double* unit_w64) {
    const PyrLevelDev& last = tab.lv[tab.n_levels - 1];
    const size_t cols = (size_t)last.xtab_off + last.zoom_w, rows = (size_t)last.ytab_off + last.zoom_h;
    ax.xbase.resize(cols); ax.xidx.resize(cols * 6); ax.xw.resize(cols * 6); ax.xw64.resize(f64 ? cols * 6 : 0);
    ax.ybase.resize(rows); ax.yidx.resize(rows * 6); ax.yw.resize(rows * 6); ax.yw64.resize(f64 ? rows * 6 : 0);
    long long unit_tiles = 0, zero_chunks = 0;
    tab.n_general = 0;
    bool tap_range_ok = true;
    for (int l = 0; l < tab.n_levels; ++l) {
        PyrLevelDev& d = tab.lv[l];
        const size_t x6 = (size_t)d.xtab_off * 6, y6 = (size_t)d.ytab_off * 6;
        int *xb = ax.xbase.data() + d.xtab_off, *yb = ax.ybase.data() + d.ytab_off, *xi = ax.xidx.data() + x6, *yi = ax.yidx.data() + y6;
        float *xwl = ax.xw.data() + x6, *ywl = ax.yw.data() + y6;
        axis_table(d.src_w, d.zoom_w, xb, xi, xwl, f64 ? ax.xw64.data() + x6 : nullptr);
        axis_table(d.src_h, d.zoom_h, yb, yi, ywl, f64 ? ax.yw64.data() + y6 : nullptr);
        // zoom factor exactly 1 <=> every output samples an integer coordinate: weights [1,26,66,26,1,~0]/120
        // (the streaming unit kernels mirror with one reflection: needs at least kMirrorNearMin source pixels per axis)
        const bool unit = d.zoom_h == d.src_h && d.zoom_w == d.src_w && std::fabs(xwl[5]) < 1e-12f &&
                          std::fabs(ywl[5]) < 1e-12f && d.src_h >= kMirrorNearMin && d.src_w >= kMirrorNearMin;
        d.kind = unit ? kPyrUnit : kPyrGeneral;
        tab.unit_tile_start[l] = (int)unit_tiles;
        tab.zero_chunk_start[l] = (int)zero_chunks;
        tab.unit_tiles_x[l] = (d.out_w + kUnitTW - 1) / kUnitTW;
        d.xreg_off = (int)ax.xreg.size();
        d.yreg_off = (int)ax.yreg.size();
        if (unit) {
            unit_tiles += (long long)tab.unit_tiles_x[l] * ((d.out_h + kUnitTH - 1) / kUnitTH);
            for (int j = 0; j < 6; ++j) unit_w[j] = xwl[j];
            if (f64)
                for (int j = 0; j < 6; ++j) unit_w64[j] = ax.xw64[x6 + j];
            continue;
        }
        ++tab.n_general;
        // scipy's mode-'constant' artefact: the last output coordinate (n_out - 1) * step can round to just above n_in - 1, and the
        // whole row / column is then cval = 0 WITHOUT a pixel being read (axis_table leaves its six weights 0) -- a NaN / inf pixel
        // under it stays out of the level.  0 * NaN would not: such a row / column leaves the resampler and joins the zero fill of
        // "canvas beyond the zoomed crop" (pyramid_zero_kernel); d.zoom_* from here on = the outputs the resampler produces
        auto dead = [](const float* w6) { return w6[0] == 0.0f && w6[1] == 0.0f && w6[2] == 0.0f && w6[3] == 0.0f && w6[4] == 0.0f && w6[5] == 0.0f; };
        if (d.zoom_w > 1 && dead(xwl + (size_t)(d.zoom_w - 1) * 6)) --d.zoom_w;
        if (d.zoom_h > 1 && dead(ywl + (size_t)(d.zoom_h - 1) * 6)) --d.zoom_h;
        const int zc = std::min(d.zoom_w, d.out_w), zr = std::min(d.zoom_h, d.out_h);
        if (!region_table(xb, xi, zc, d.src_x0, tab.regions_x, region_w(tab.C), kRegionHaloL, kRegionHaloR, ax.xreg)) tap_range_ok = false;
        if (!region_table(yb, yi, zr, d.src_y0, tab.regions_y, region_h(tab.C), kRegionHaloT, kRegionHaloB, ax.yreg)) tap_range_ok = false;
        zero_chunks += (pyramid_zero_count(d.zoom_h, d.zoom_w, d.out_h, d.out_w) + 1023) / 1024;   // (exactly the pixels the resampler leaves)
    }
    tab.unit_tile_start[tab.n_levels] = (int)unit_tiles;
    tab.unit_tiles_per_frame = (int)unit_tiles;
    tab.zero_chunk_start[tab.n_levels] = (int)zero_chunks;
    tab.zero_chunks_per_frame = (int)zero_chunks;
    if (ax.xreg.empty()) ax.xreg.push_back(0);
    if (ax.yreg.empty()) ax.yreg.push_back(0);
    return tap_range_ok;
}
// The unit level of a "classic" plan -- exactly one unit level, its canvas at least as large as its crop, and 1 - 7 general levels that
// all resample that crop -- or -1.
inline int same_crop_unit(const PyrTab& tab) {
    int unit = -1, n_unit = 0;
    for (int l = 0; l < tab.n_levels; ++l)
        if (tab.lv[l].kind == kPyrUnit) { unit = l; ++n_unit; }
    if (n_unit != 1 || tab.n_general < 1 || tab.n_general > 7) return -1;
    const PyrLevelDev& u = tab.lv[unit];
    if (u.out_h < u.src_h || u.out_w < u.src_w) return -1;
    for (int l = 0; l < tab.n_levels; ++l) {
        const PyrLevelDev& d = tab.lv[l];
        if (d.kind == kPyrGeneral && !(d.src_y0 == u.src_y0 && d.src_x0 == u.src_x0 && d.src_h == u.src_h && d.src_w == u.src_w)) return -1;
    }
    return unit;
}
// finest level first: the column records' capacity per wave tile shrinks with the position (w3_rec_cap)
inline std::vector<int> finest_first(const PyrTab& tab, std::vector<int> levels) {
    std::stable_sort(levels.begin(), levels.end(), [&](int x, int y) {
        return (double)tab.lv[x].zoom_w / tab.lv[x].src_w > (double)tab.lv[y].zoom_w / tab.lv[y].src_w;
    });
    return levels;
}

// ------------------------------------------------------------------------------------------ the gray stream path
// Row programs and column records of the single-read stream kernels (gray_stream_kernel) for the classic plan on unit level `unit`, in
// slot layout `layout` (silent_gray.h, stream_slots: 0 for ladders of ratio >= e^.5, 1 ("dense", kernels for 7 levels only) down to 1.4;
// F64 plans: every layout -- the F64 stream kernels spill nothing to scratch).  False where the layout cannot hold
// the plan: a level's step is too small for its vertical slots.  st: px_off / out_w of the levels visited; on success G, tiles_y, waves_x.
struct StreamTables { std::vector<int> prog, hdr, rec; };
inline bool build_stream_tables(const PyrTab& tab, const AxisTables& ax, int unit, int layout, bool f64, StreamTables& out, StreamTab& st) {
    bool ok = true;
    const PyrLevelDev& u = tab.lv[unit];
    const int G = tab.n_general;
    const int tiles_y = (u.out_h + kFusedTH - 1) / kFusedTH;
    const int waves_x = ((u.out_w + kFusedTW - 1) / kFusedTW) * kFusedWaves;
    const int Gp = layout ? 7 : stream_pad_levels(G), PR = kStreamProgRow(layout, Gp, f64), RI = stream_rec_ints(f64);
    const size_t n_rec = (size_t)tiles_y * kStreamRows;
    std::vector<int>&prog = out.prog, &hdr = out.hdr, &rec = out.rec;
    prog.assign(n_rec * PR, 0);
    hdr.assign((size_t)G * waves_x * 2, 0);
    rec.assign((size_t)G * waves_x * 64 * RI, 0);
    for (size_t r = 0; r < n_rec; ++r)
        for (int gg = 0; gg < Gp; ++gg) prog[r * PR + gg] = 7 << stream_done_shift(layout);  // inert: feeds nothing, no slot completes
    std::vector<char> used(n_rec * G * kStreamSlots, 0);
    int g = 0;
    for (int l = 0; l < tab.n_levels && ok; ++l) {
        const PyrLevelDev& d = tab.lv[l];
        if (d.kind != kPyrGeneral) continue;
        const int zc = std::min(d.zoom_w, d.out_w), zr = std::min(d.zoom_h, d.out_h);
        const int* yb = ax.ybase.data() + d.ytab_off;
        const int* xb = ax.xbase.data() + d.xtab_off;
        for (int oy = 0; oy < zr && ok; ++oy) {
            const int t = yb[oy] / kFusedTH;
            if (yb[oy] < 0 || t >= tiles_y) { ok = false; break; }
            const int slot = oy % stream_slots(layout, g);
            for (int j = 0; j < 6; ++j) {
                const int i = yb[oy] - t * kFusedTH + 2 + j;  // stream row of tap j (a tile streams rows y0-4 ..)
                if (i < 0 || i >= kStreamRows) { ok = false; break; }
                const size_t r = (size_t)t * kStreamRows + i;
                const size_t e = r * G + g;
                if (used[e * kStreamSlots + slot]) { ok = false; break; }  // two live rows in one slot: step too small
                used[e * kStreamSlots + slot] = 1;
                int* pr = prog.data() + r * PR;
                int& meta = pr[g];
                if (f64) std::memcpy(pr + stream_w_off(layout, Gp, g, true) + 2 * slot, &ax.yw64[(size_t)(d.ytab_off + oy) * 6 + j], 8);
                else std::memcpy(pr + stream_w_off(layout, Gp, g) + slot, &ax.yw[(size_t)(d.ytab_off + oy) * 6 + j], 4);
                meta |= 128;  // this stream row feeds level g
                if (j == 0) meta |= 1 << slot;
                if (j == 5) {
                    const int ds = stream_done_shift(layout);
                    if (((meta >> ds) & 7) != 7) { ok = false; break; }  // two rows completing together
                    meta = (meta & ~(7 << ds)) | (slot << ds) | (oy << stream_row_shift(layout));
                }
            }
        }
        int ox = 0;
        for (int wx = 0; wx < waves_x && ok; ++wx) {
            const int xw0 = wx * kFusedCols;
            while (ox < zc && xb[ox] < xw0) ++ox;
            int n = 0;
            while (ox + n < zc && xb[ox + n] < xw0 + kFusedCols) ++n;
            if (n > 64) { ok = false; break; }
            hdr[((size_t)g * waves_x + wx) * 2] = ox;
            hdr[((size_t)g * waves_x + wx) * 2 + 1] = n;
            for (int j = 0; j < n; ++j) {
                int* r = rec.data() + (((size_t)g * waves_x + wx) * 64 + j) * RI;
                r[0] = xb[ox + j] - xw0 + 2;  // lane holding tap 0 (lane 0 <-> column xw0 - 4)
                if (r[0] < 0 || r[0] + 5 > 63) { ok = false; break; }
                if (f64) std::memcpy(r + 2, &ax.xw64[(size_t)(d.xtab_off + ox + j) * 6], 48);
                else std::memcpy(r + 1, &ax.xw[(size_t)(d.xtab_off + ox + j) * 6], 24);
            }
            ox += n;
        }
        st.px_off[g] = tab.px_off[l];
        st.out_w[g] = d.out_w;
        ++g;
    }
    if (!ok) return false;
    st.G = G; st.tiles_y = tiles_y; st.waves_x = waves_x;
    return true;
}

// ------------------------------------------------------------------------------------------ the RGB walk
// Walk plans of pyramid_walk3_kernel (3 channels).  Classic pyramid (one unit level whose crop every other level resamples): one plan.
// Anything else (the reference's nested centre crops): a unit level alone; and the general levels
// either as ONE "union" plan -- the walk over the OUTERMOST crop serves every level whose crop lies inside it, wherever an
// output's 6 x 6 taps stay inside that level's own crop (no mirroring: the frame pixels ARE the taps); the inner levels' first /
// last output rows and columns go to pyramid_border_kernel -- or, where that is not eligible, one plan per level on its own crop.
// Per plan: a row program (one record per source row of the crop: "an output row of level g completes here" + its 6 vertical
// weights) and column records per PX-pixel wave tile.
// A classic pyramid of more than 7 general levels stays on the unit + region kernels: the levels beyond the seventh as walk plans
// of their own, or left to pyramid_region_kernel behind the walk, cost a second pass over the frame for a few small levels
// (32 x 1080p, sqrt 2, 12 levels: 1.38 / 1.35 ms against 1.27 ms; profiles/r05_experiments.txt).
struct WalkSpec {
    int unit;                 // level index of the plan's unit level, or -1
    int crop;                 // the level whose crop the plan walks
    std::vector<int> gen;     // its general levels (union plans: finest first; those other than `crop` interior-only)
};
typedef std::vector<WalkSpec> WalkCandidate;    // the plans of one launch
// The candidates of a 3-channel plan in the order they are tried (tune: the PYRAMID knob, bit 4 forbids the union plan)
inline std::vector<WalkCandidate> walk_candidates(const PyrTab& tab, unsigned tune) {
    std::vector<WalkCandidate> candidates;
    std::vector<int> gens;
    WalkCandidate units;
    for (int l = 0; l < tab.n_levels; ++l) {
        if (tab.lv[l].kind == kPyrUnit) units.push_back(WalkSpec{l, l, {}});
        else gens.push_back(l);
    }
    const int unit = same_crop_unit(tab);
    if (unit >= 0) {
        candidates.push_back({WalkSpec{unit, unit, finest_first(tab, gens)}});
    } else {
        // the union: an outermost general level whose crop holds every other general level's crop
        int outer = -1;
        for (int o : gens) {
            bool holds = true;
            for (int l : gens) {
                const PyrLevelDev &a = tab.lv[o], &d = tab.lv[l];
                holds = holds && d.src_y0 >= a.src_y0 && d.src_x0 >= a.src_x0 && d.src_y0 + d.src_h <= a.src_y0 + a.src_h &&
                        d.src_x0 + d.src_w <= a.src_x0 + a.src_w;
            }
            if (holds) { outer = o; break; }
        }
        if (outer >= 0 && gens.size() >= 2 && gens.size() <= 7 && !(tune & 4u)) {
            candidates.push_back(units);
            candidates.back().push_back(WalkSpec{-1, outer, finest_first(tab, gens)});
        }
        candidates.push_back(units);
        for (int l : gens) candidates.back().push_back(WalkSpec{-1, l, {l}});
    }
    return candidates;
}
// The tables of one candidate at PX pixels per consumer wave: all row programs, column headers and records in ONE blob (256-byte aligned
// parts), the kernel's arguments but for the device pointers and the per-launch decomposition, the border outputs of a union plan.  False
// where no walk serves the candidate (too many plans, a unit canvas smaller than its crop, a crop under 8 columns) or PX is too wide for
// a level's zoom step (the caller tries the next narrower one).
struct WalkTables {
    std::vector<int> blob;
    std::vector<size_t> offs;   // [plan][3]: row program, column headers, column records of the plan in the blob, in ints
    int Gp;                   // general levels the kernel is instantiated for (4 or 7)
    Walk3Args args;
    BorderTab border;
};
inline bool build_walk_tables(const PyrTab& tab, const AxisTables& ax, const WalkCandidate& hp, int px, const float* unit_w, WalkTables& out) {
    if (hp.empty() || (int)hp.size() > kW3MaxPlans) return false;
    int maxg = 0;
    for (const WalkSpec& h : hp) {
        const PyrLevelDev& c = tab.lv[h.crop];   // (a plan with a unit level walks that level's crop: its canvas at least as large)
        if ((h.unit >= 0 && (c.out_h < c.src_h || c.out_w < c.src_w)) || c.src_w < 8) return false;
        maxg = std::max(maxg, (int)h.gen.size());
    }
    const int Gp = stream_pad_levels(std::max(maxg, 1)), PR = w3_prog_row(Gp);
    const int rec_total = w3_rec_total(px, Gp);
    std::vector<int>& blob = out.blob;                        // all tables of all plans, offsets in ints
    Walk3Args& wa = out.args;
    std::memset(&wa, 0, sizeof(wa));
    BorderTab& bt = out.border;
    std::memset(&bt, 0, sizeof(bt));
    for (size_t pi = 0; pi < hp.size(); ++pi) {
        const WalkSpec& h = hp[pi];
        const PyrLevelDev& c = tab.lv[h.crop];
        const int walk_h = h.unit >= 0 ? c.out_h : c.src_h;
        int walk_w = h.unit >= 0 ? c.out_w : c.src_w;
        const int G = (int)h.gen.size();
        // A last strip that holds a sliver of the crop costs a whole strip of row steps (the reference layout on 1080p: 10
        // of 128 pixels, one block in eleven).  Plans of general levels only give it up: the few output columns anchored in
        // it join the border pixels (pyramid_border_px: taps straight from the frame), the walk ends at the strip boundary --
        // the pixels behind it are still in the frame for the last strip's halo.
        const int strip_px = kW3NC * px;
        if (h.unit < 0 && G >= 2 && walk_w > strip_px && walk_w % strip_px != 0 && walk_w % strip_px <= px / 2)
            walk_w -= walk_w % strip_px;
        const int waves_x = ((walk_w + kW3NC * px - 1) / (kW3NC * px)) * kW3NC;
        const size_t n_rec = (size_t)walk_h + 8;                 // stream rows y = -4 .. walk_h + 3 at index y + 4
        const size_t n_rec_pad = n_rec + 2 * kWalkCH;            // the loader fetches whole chunks of records
        std::vector<int> prog(n_rec_pad * PR, 0), hdr((size_t)std::max(G, 1) * waves_x * 2, 0), rec((size_t)waves_x * rec_total * 8, 0);
        Walk3Plan& wp3 = wa.plan[pi];
        for (int g = 0; g < G; ++g) {
            const PyrLevelDev& d = tab.lv[h.gen[g]];
            const int zc = std::min(d.zoom_w, d.out_w), zr = std::min(d.zoom_h, d.out_h);
            const int* yb = ax.ybase.data() + d.ytab_off;
            const int* xb = ax.xbase.data() + d.xtab_off;
            // a level on ANOTHER crop than the walk's: offset of its crop inside the walk, and the outputs whose taps
            // (rows / columns base - 2 .. base + 3) stay inside its own crop
            const int dy = d.src_y0 - c.src_y0, dx = d.src_x0 - c.src_x0;
            int oy_lo = 0, oy_hi = zr, ox_lo = 0, ox_hi = zc;
            if (d.src_y0 != c.src_y0 || d.src_x0 != c.src_x0 || d.src_h != c.src_h || d.src_w != c.src_w) {
                while (oy_lo < zr && yb[oy_lo] - 2 < 0) ++oy_lo;
                while (oy_hi > oy_lo && yb[oy_hi - 1] + 3 > d.src_h - 1) --oy_hi;
                while (ox_lo < zc && xb[ox_lo] - 2 < 0) ++ox_lo;
                while (ox_hi > ox_lo && xb[ox_hi - 1] + 3 > d.src_w - 1) --ox_hi;
            }
            while (ox_hi > ox_lo && xb[ox_hi - 1] + dx >= walk_w) --ox_hi;   // anchored behind a trimmed walk
            if (oy_lo > 0 || oy_hi < zr || ox_lo > 0 || ox_hi < zc) {
                if (oy_hi <= oy_lo || ox_hi <= ox_lo || bt.n >= kMaxLevels) return false;
                BorderLevel& bl = bt.lv[bt.n++];
                bl.level = h.gen[g];
                bl.oy_lo = oy_lo; bl.oy_hi = oy_hi; bl.ox_lo = ox_lo; bl.ox_hi = ox_hi;
                bl.zr = zr; bl.zc = zc;
                bl.start = bt.per_frame;
                bt.per_frame += zr * zc - (oy_hi - oy_lo) * (ox_hi - ox_lo);
            }
            for (int oy = oy_lo; oy < oy_hi; ++oy) {
                // one record entry per COMPLETING row: flag + output row, 6 weights
                const int y = yb[oy] + dy;
                if (y < 0 || y >= walk_h) return false;
                const size_t r = (size_t)(y + 7);                // the last tap sits on stream row y + 3, index y + 4
                if (r >= n_rec) return false;
                int* pr = prog.data() + r * PR;
                if (pr[g] & 1) return false;                     // two rows of one level completing together: step < 1
                pr[g] = 1 | (oy << 8);
                std::memcpy(pr + Gp + 6 * g, &ax.yw[(size_t)(d.ytab_off + oy) * 6], 24);
            }
            int ox = ox_lo;
            for (int wx = 0; wx < waves_x; ++wx) {
                const int xw0 = wx * px;
                while (ox < ox_hi && xb[ox] + dx < xw0) ++ox;
                int n = 0;
                while (ox + n < ox_hi && xb[ox + n] + dx < xw0 + px) ++n;
                if (n > w3_rec_cap(px, g)) return false;         // outputs per wave tile (the gather takes <= 21)
                hdr[((size_t)g * waves_x + wx) * 2] = ox;
                hdr[((size_t)g * waves_x + wx) * 2 + 1] = n;
                for (int j = 0; j < n; ++j) {
                    int* r = rec.data() + ((size_t)wx * rec_total + w3_rec_base(px, g) + j) * 8;
                    r[0] = (xb[ox + j] + dx - xw0) * 3;          // FLOAT index of tap 0, channel 0 (line starts at pixel xw0 - 2)
                    if (r[0] < 0 || r[0] + 2 + 15 > kW3TileF - 1) return false;
                    std::memcpy(r + 1, &ax.xw[(size_t)(d.xtab_off + ox + j) * 6], 24);
                }
                ox += n;
            }
            wp3.pyr.px_off[g] = tab.px_off[h.gen[g]];
            wp3.pyr.out_w[g] = d.out_w;
        }
        wp3.src_y0 = c.src_y0; wp3.src_x0 = c.src_x0; wp3.src_h = c.src_h; wp3.src_w = c.src_w;
        wp3.shift = tab.W % 4 ? 0 : (c.src_x0 * 3) % 4;   // (other widths: the loader fetches single floats, not 16-byte groups)
        wp3.has_unit = h.unit >= 0 ? 1 : 0;
        wp3.out_h = walk_h; wp3.out_w = walk_w;
        wp3.eff_h = h.unit >= 0 ? std::min(c.zoom_h, c.out_h) : walk_h;
        wp3.eff_w = h.unit >= 0 ? std::min(c.zoom_w, c.out_w) : walk_w;
        wp3.px_off = h.unit >= 0 ? tab.px_off[h.unit] : 0;
        wp3.pyr.G = G;
        auto put = [&](const std::vector<int>& v) {
            blob.resize((blob.size() + 63) / 64 * 64, 0);        // 256-byte aligned tables
            blob.insert(blob.end(), v.begin(), v.end());
            return blob.size() - v.size();
        };
        out.offs.insert(out.offs.end(), {put(prog), put(hdr), put(rec)});
    }
    wa.H = tab.H; wa.W = tab.W;
    wa.n_plans = (int)hp.size();
    wa.frame_px = tab.frame_px_out;
    for (int j = 0; j < 6; ++j) wa.wx[j] = unit_w[j];
    out.Gp = Gp;
    return true;
}

}  // namespace silent
