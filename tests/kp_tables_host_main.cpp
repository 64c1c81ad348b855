// Stand-alone driver of the keypoint tail's host planning (pysilent_amd/csrc/silent_peaks_plan.h, and region_prepare / select_prepare of
// silent_peaks_api.hip) on the library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("kp_tables")): what the tail PLANS, as text.
// ONE translation unit with silent_unity.hip, -DSILENT_HOST_ONLY, under -fsanitize=address,undefined; launches are compiled out.
//   no argument      cases on stdin, one per line:
//                        name n_frames sparse_th pv_ws reserve n_levels <h w rh rw per level>
//                    Each case runs region_prepare (with `reserve`) and select_prepare (with `sparse_th`, `pv_ws`), each on a fresh context,
//                    and prints: the status (and silent_last_error on a refusal); every field of every RegionLevel; general and the
//                    two per-frame table sizes; the SumTab; the block counts of the LevelTabs; every KeypointWs pointer as its offset into
//                    the workspace; the zero range, n_cells and the workspace's capacity (a fresh context's is total + total / 4 + 2^20):
//                    tests/golden/kp_tables.txt.  Every accepted case is also CHECKED: the pieces are 256-aligned, pairwise disjoint and
//                    inside the total, the zero range is exactly chunk_counts | hit_masks | cand_n | nan_flags, zero_bytes is a multiple
//                    of 16 -- exit status 1 otherwise.
//   --cells          build_cell_tab cases:  name rh rw n_levels <h w per level>
//   --boost          the boost parameters:  name recovery_mode exhaustion_max excitation_max amount percentage visualize
//                    (a name that starts with "null" passes NULL)
//   --layout         the same case lines as the first form, for sizes nobody can allocate: the pure layout function alone, the same
//                    checks, one "ok" line per case (nothing of it is recorded)
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#ifndef SILENT_HOST_ONLY
#error "host-only build: compile with -DSILENT_HOST_ONLY (no GPU is touched)"
#endif
#include "../pysilent_amd/csrc/silent_unity.hip"

// ---- the names of silent_peaks_api.hip / silent_peaks_plan.h this driver touches beyond region_prepare / select_prepare, RegionPlan /
// SelectPlan's tab, blocks, cblocks, rt, general, w, stab, sblocks, mm, nmm, st and the members of KeypointWs: a rename there is an edit of
// these lines (the block as it read when tests/golden/kp_tables.txt was recorded: profiles/kp_tail/README.md)
static long long reduction_blocks(const SelectPlan& sp) { return sp.cblocks; }
static int cell_tab_of(silent_ctx* ctx, const char* who, const silent_extent* levels, int n_levels, int rh, int rw, silent::CellTab* ct) {
    return refuse(ctx, who, silent::build_cell_tab(levels, n_levels, rh, rw, ct));
}
static int boost_of(silent_ctx* ctx, const silent_boosting_params* p, silent::BoostP* bp) { return refuse(ctx, "silent_boosting_step", silent::boost_params(p, bp)); }
struct LayoutOffsets {   // a select_prepare's tables and, as byte offsets (-1: none), the pieces the pure layout function gives them
    long long off[12];   // cells chunk_counts hit_masks cand_n nan_flags chunk_offsets m1 pooled sum cand dense_flags pv
    size_t reserve, zero_from, zero_bytes, n_cells, total;
    long long blocks, sum_entries, pv_px;
    bool general;
    silent::RegionTab rt;
};
static int layout_of(silent_ctx* ctx, const char* who, const silent_extent* levels, const silent_extent* regions, int n_levels, int n_frames, int sparse_th,
                     bool pv_ws, LayoutOffsets* lo) {
    SelectPlan sp;   // select_prepare without its workspace and launches
    TRY(build_level_tab(ctx, who, levels, n_levels, n_frames, silent::kSelTW, silent::kSelTH, &sp.stab, &sp.sblocks));
    TRY(region_tables(ctx, who, levels, n_levels, n_frames, regions, &sp));
    silent::build_sum_tab(levels, n_levels, n_frames, sparse_th, sp.general, &sp.st);
    lo->reserve = sizeof(unsigned) * 2 * (size_t)n_frames * n_levels;
    lo->blocks = sp.blocks; lo->sum_entries = sp.st.frame_entries; lo->pv_px = pv_ws ? sp.tab.frame_px : 0; lo->general = sp.general; lo->rt = sp.rt;
    const silent::KeypointLayout k = silent::keypoint_layout(n_levels, n_frames, lo->blocks, lo->reserve, lo->rt, lo->general, lo->sum_entries, lo->pv_px);
    const size_t off[12] = {k.cells, k.chunk_counts, k.hit_masks, k.cand_n, k.nan_flags, k.chunk_offsets, k.m1, k.pooled, k.sum, k.cand, k.dense_flags, k.pv};
    for (int i = 0; i < 12; ++i) lo->off[i] = (long long)off[i];
    if (!lo->sum_entries) lo->off[8] = lo->off[9] = -1;
    if (!lo->pv_px) lo->off[11] = -1;
    lo->zero_from = k.zero_from; lo->zero_bytes = k.zero_bytes; lo->n_cells = k.n_cells; lo->total = k.total;
    return SILENT_OK;
}
// ----

struct Case {
    std::string name;
    int n_frames, sparse_th, pv_ws, n_levels;
    size_t reserve;
    std::vector<silent_extent> levels, regions;
};
static bool parse(const std::string& line, Case* c) {
    std::istringstream in(line);
    if (!(in >> c->name >> c->n_frames >> c->sparse_th >> c->pv_ws >> c->reserve >> c->n_levels)) return false;
    c->levels.clear();
    c->regions.clear();
    int h, w, rh, rw;
    while (in >> h >> w >> rh >> rw) {
        c->levels.push_back(silent_extent{h, w});
        c->regions.push_back(silent_extent{rh, rw});
    }
    if (c->levels.empty()) {   // (n_levels 0: pointers that are not NULL)
        c->levels.push_back(silent_extent{1, 1});
        c->regions.push_back(silent_extent{1, 1});
    }
    return true;
}

static std::string text;     // the line being built
static void put(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void put(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    text += buf;
}
static void emit() {
    std::printf("%s\n", text.c_str());
    text.clear();
}
static unsigned bits(float f) {
    unsigned b;
    std::memcpy(&b, &f, 4);
    return b;
}
static void put_ints(const char* what, const int* v, int n) {
    put(" | %s", what);
    for (int i = 0; i < n; ++i) put(" %d", v[i]);
}

static void put_region_levels(const std::string& head, const silent::RegionTab& rt, int n_levels) {
    for (int l = 0; l < n_levels; ++l) {
        const silent::RegionLevel& r = rt.lv[l];
        text = head;
        put(" L%d | %d %d %d %d", l, r.oh, r.ow, r.nrs, r.ncs);
        put_ints("rcut", r.rcut, silent::kMaxSeg + 1);
        put_ints("ccut", r.ccut, silent::kMaxSeg + 1);
        put_ints("wy_lo", r.wy_lo, silent::kMaxWin);
        put_ints("wy_hi", r.wy_hi, silent::kMaxWin);
        put_ints("wx_lo", r.wx_lo, silent::kMaxWin);
        put_ints("wx_hi", r.wx_hi, silent::kMaxWin);
        put(" | %d %d %d %d %lld %lld | scale %08x %08x", r.ry, r.rx, r.pad_y, r.pad_x, r.m1_off, r.pooled_off, bits(r.yscale), bits(r.xscale));
        emit();
    }
}

// ---- the pieces of a keypoint workspace and what must hold of them
struct Piece {
    const char* name;
    long long off;     // -1: none
    size_t bytes;      // what the piece must hold (this driver's own arithmetic)
    bool zeroed;
};
static size_t up256(size_t v) { return (v + 255) / 256 * 256; }
static int n_pieces(const Case& c, long long blocks, const silent::RegionTab& rt, bool general, long long sum_entries, long long pv_px,
                    const long long* off, Piece* p) {
    const size_t nf = (size_t)c.n_frames, nl = (size_t)c.n_levels;
    const Piece all[12] = {
        {"cells", off[0], nf * nl * silent::kCells * sizeof(unsigned), false},
        {"chunk_counts", off[1], (size_t)blocks * sizeof(int), true},
        {"hit_masks", off[2], (size_t)blocks * 4 * silent::kKpPer * sizeof(unsigned long long), true},
        {"cand_n", off[3], nf * sizeof(int), true},
        {"nan_flags", off[4], nf * nl * sizeof(int), true},
        {"chunk_offsets", off[5], (size_t)blocks * sizeof(long long), false},
        {"m1", off[6], general ? nf * (size_t)rt.m1_per_frame * sizeof(float) : 0, false},
        {"pooled", off[7], general ? nf * (size_t)rt.pooled_per_frame * sizeof(float) : 0, false},
        {"sum", off[8], (size_t)sum_entries * nf * sizeof(float), false},
        {"cand", off[9], sum_entries ? nf * silent::kCandCap * sizeof(silent::Candidate) : 0, false},
        {"dense_flags", off[10], nf * nl * sizeof(int), false},
        {"pv", off[11], (size_t)pv_px * nf * sizeof(float), false},
    };
    for (int i = 0; i < 12; ++i) p[i] = all[i];
    return 12;
}
// aligned, disjoint, inside [reserve, total); the zero range = the union of the zeroed pieces (each rounded up to 256) and nothing else
static bool check_pieces(const char* name, const Piece* p, int n, size_t reserve, size_t total, size_t zero_from, size_t zero_bytes) {
    bool ok = true;
    auto bad = [&](const char* what, const char* piece) {
        std::printf("CHECK FAILED %s: %s (%s)\n", name, what, piece);
        ok = false;
    };
    size_t zlo = (size_t)-1, zhi = 0, zsum = 0;
    for (int i = 0; i < n; ++i) {
        if (p[i].off < 0) continue;
        const size_t a = (size_t)p[i].off, b = a + p[i].bytes;
        if (a % 256) bad("not 256-aligned", p[i].name);
        if (a < reserve || b > total) bad("outside the workspace", p[i].name);
        for (int j = 0; j < i; ++j) {
            if (p[j].off < 0 || !p[i].bytes || !p[j].bytes) continue;
            const size_t c = (size_t)p[j].off, d = c + p[j].bytes;
            if (a < d && c < b) bad("overlaps another piece", p[i].name);
        }
        if (p[i].zeroed) {
            zlo = std::min(zlo, a);
            zhi = std::max(zhi, a + up256(p[i].bytes));
            zsum += up256(p[i].bytes);
        } else if (p[i].bytes && a < zero_from + zero_bytes && zero_from < b) {
            bad("lies inside the zero range", p[i].name);
        }
    }
    if (zero_from != zlo || zero_from + zero_bytes != zhi || zero_bytes != zsum) bad("the zero range is not the union of the zeroed pieces", "zero");
    if (zero_bytes % 16) bad("zero_bytes is not a multiple of 16", "zero");
    return ok;
}

static void put_ws(const silent_ctx* ctx, const KeypointWs& w, long long* off) {
    const void* ptr[12] = {w.cells, w.chunk_counts, w.hit_masks, w.cand_n, w.nan_flags, w.chunk_offsets, w.m1, w.pooled, w.sum, w.cand, w.dense_flags, w.pv};
    static const char* const names[12] = {"cells", "chunk_counts", "hit_masks", "cand_n", "nan_flags", "chunk_offsets", "m1", "pooled", "sum", "cand", "dense_flags", "pv"};
    put(" | ws");
    for (int i = 0; i < 12; ++i) {
        off[i] = ptr[i] ? (long long)((const char*)ptr[i] - (const char*)ctx->ws.p) : -1;
        if (ptr[i]) put(" %s %lld", names[i], off[i]);
        else put(" %s null", names[i]);
    }
    put(" | zero %lld %zu n_cells %zu | cap %zu", w.zero_from ? (long long)((const char*)w.zero_from - (const char*)ctx->ws.p) : -1, w.zero_bytes, w.n_cells,
        ctx->ws.cap);
}
// (a fresh context's workspace: cap = total + total / 4 + 2^20, total a multiple of 256)
static size_t total_of(size_t cap) { return (cap - (1u << 20)) / 5 * 4; }

static bool tables_case(const Case& c) {
    bool ok = true;
    const char* who = "kp_tables";
    {
        silent_ctx* ctx = nullptr;
        if (silent_create(0, &ctx) != SILENT_OK) return false;
        RegionPlan rp;
        const int rc = region_prepare(ctx, who, c.levels.data(), c.n_levels, c.n_frames, c.regions.data(), c.reserve, nullptr, &rp);
        const std::string head = c.name + " region";
        text = head;
        put(" | %d", rc);
        if (rc != SILENT_OK) {
            put(" | %s", silent_last_error(ctx));
            emit();
        } else {
            emit();
            put_region_levels(head, rp.rt, c.n_levels);
            text = head;
            put(" | general %d m1 %lld pooled %lld | blocks %lld %lld", (int)rp.general, rp.rt.m1_per_frame, rp.rt.pooled_per_frame, rp.blocks, rp.cblocks);
            long long off[12];
            put_ws(ctx, rp.w, off);
            emit();
            Piece p[12];
            const int n = n_pieces(c, rp.blocks, rp.rt, rp.general, 0, 0, off, p);
            ok = check_pieces(head.c_str(), p, n, c.reserve, total_of(ctx->ws.cap), (size_t)((const char*)rp.w.zero_from - (const char*)ctx->ws.p), rp.w.zero_bytes) && ok;
        }
        silent_destroy(ctx);
    }
    {
        silent_ctx* ctx = nullptr;
        if (silent_create(0, &ctx) != SILENT_OK) return false;
        SelectPlan sp;
        const int rc = select_prepare(ctx, who, c.levels.data(), c.n_levels, c.n_frames, c.regions.data(), nullptr, &sp, c.sparse_th, c.pv_ws != 0);
        const std::string head = c.name + " select";
        text = head;
        put(" | %d", rc);
        if (rc != SILENT_OK) {
            put(" | %s", silent_last_error(ctx));
            emit();
        } else {
            emit();
            put_region_levels(head, sp.rt, c.n_levels);
            text = head;
            put(" | general %d m1 %lld pooled %lld | blocks %lld %lld %lld | nmm %d mm %lld", (int)sp.general, sp.rt.m1_per_frame, sp.rt.pooled_per_frame,
                reduction_blocks(sp), sp.sblocks, sp.blocks, sp.nmm, (long long)((const char*)sp.mm - (const char*)ctx->ws.p));
            put(" | sum %d %d", sp.st.th, sp.st.gpt);
            for (int l = 0; l <= silent::kMaxLevels; ++l) put(" %lld", sp.st.off[l]);
            put(" entries %lld", sp.st.frame_entries);
            long long off[12];
            put_ws(ctx, sp.w, off);
            emit();
            Piece p[12];
            const size_t reserve = sizeof(unsigned) * 2 * (size_t)sp.nmm;
            const int n = n_pieces(c, sp.blocks, sp.rt, sp.general, sp.st.frame_entries, c.pv_ws ? sp.tab.frame_px : 0, off, p);
            ok = check_pieces(head.c_str(), p, n, reserve, total_of(ctx->ws.cap), (size_t)((const char*)sp.w.zero_from - (const char*)ctx->ws.p), sp.w.zero_bytes) && ok;
        }
        silent_destroy(ctx);
    }
    return ok;
}

// the pure layout on sizes that cannot be allocated: the same checks, nothing recorded
static int layout_case(silent_ctx* ctx, const Case& c) {
    LayoutOffsets lo;
    const int rc = layout_of(ctx, "kp_tables", c.levels.data(), c.regions.data(), c.n_levels, c.n_frames, c.sparse_th, c.pv_ws != 0, &lo);
    if (rc != SILENT_OK) {
        std::printf("%s layout | %d | %s\n", c.name.c_str(), rc, rc == -100 ? "no pure layout function in this build" : silent_last_error(ctx));
        return 1;
    }
    Piece p[12];
    const int n = n_pieces(c, lo.blocks, lo.rt, lo.general, lo.sum_entries, lo.pv_px, lo.off, p);
    if (!check_pieces(c.name.c_str(), p, n, lo.reserve, lo.total, lo.zero_from, lo.zero_bytes)) return 1;
    std::printf("%s layout | ok | total %zu zero %zu %zu entries %lld\n", c.name.c_str(), lo.total, lo.zero_from, lo.zero_bytes, lo.sum_entries);
    return 0;
}

static int cells_mode(silent_ctx* ctx) {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name;
        int rh, rw, n_levels, h, w;
        if (!(in >> name >> rh >> rw >> n_levels)) return 2;
        std::vector<silent_extent> levels;
        while (in >> h >> w) levels.push_back(silent_extent{h, w});
        silent::CellTab ct;
        const int rc = cell_tab_of(ctx, "kp_tables", levels.data(), n_levels, rh, rw, &ct);
        text = name;
        put(" cells | %d", rc);
        if (rc != SILENT_OK) {
            put(" | %s", silent_last_error(ctx));
        } else {
            put(" | %d %d", ct.rh, ct.rw);
            for (int l = 0; l < n_levels; ++l)
                put(" | L%d %d %d %d %d %lld %08x %08x", l, ct.oh[l], ct.ow[l], ct.y_first[l], ct.x_first[l], ct.cell_off[l], bits(ct.yscale[l]), bits(ct.xscale[l]));
            put(" | frame_cells %lld", ct.frame_cells);
        }
        emit();
    }
    return 0;
}

static int boost_mode(silent_ctx* ctx) {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name;
        silent_boosting_params p;
        if (!(in >> name >> p.recovery_mode >> p.exhaustion_max >> p.excitation_max >> p.recovery_amount >> p.recovery_percentage >> p.visualize)) return 2;
        silent::BoostP bp;
        std::memset(&bp, 0, sizeof(bp));
        const int rc = boost_of(ctx, name.rfind("null", 0) == 0 ? nullptr : &p, &bp);
        text = name;
        put(" boost | %d", rc);
        if (rc != SILENT_OK) put(" | %s", silent_last_error(ctx));
        else
            put(" | lo %08x hi %08x mode %d amount %08x percentage %08x visualize %d normer %08x centerer %08x", bits(bp.lo), bits(bp.hi), bp.recovery_mode,
                bits(bp.recovery_amount), bits(bp.recovery_percentage), bp.visualize, bits(bp.normer), bits(bp.centerer));
        emit();
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    int rc = 0;
    if (mode == "--cells" || mode == "--boost" || mode == "--layout") {
        silent_ctx* ctx = nullptr;
        if (silent_create(0, &ctx) != SILENT_OK) {
            std::printf("silent_create failed\n");
            return 2;
        }
        if (mode == "--cells") rc = cells_mode(ctx);
        else if (mode == "--boost") rc = boost_mode(ctx);
        else {
            std::string line;
            Case c;
            while (std::getline(std::cin, line)) {
                if (line.empty()) continue;
                if (!parse(line, &c)) { rc = 2; break; }
                rc = layout_case(ctx, c) ? 1 : rc;
            }
        }
        silent_destroy(ctx);
    } else if (mode.empty()) {
        std::string line;
        Case c;
        while (std::getline(std::cin, line)) {
            if (line.empty()) continue;
            if (!parse(line, &c)) { rc = 2; break; }
            if (!tables_case(c)) rc = 1;
        }
    } else {
        rc = 2;
    }
    if (rc == 2) std::printf("usage: [--cells | --boost | --layout] < case lines (see the head of tests/kp_tables_host_main.cpp)\n");
    return rc;
}
