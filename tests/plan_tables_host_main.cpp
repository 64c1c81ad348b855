// Stand-alone driver of silent_pyramid_plan_create_ex on the library's HOST side (pysilent_amd/csrc/build.py,
// build_host_driver("plan_tables")): what the planner BUILDS, as text.  ONE translation unit with silent_unity.hip, -DSILENT_HOST_ONLY,
// under -fsanitize=address,undefined: device memory is host memory (calloc), so every table of a plan can be read back.
//   no argument      plan descriptions on stdin, one per line:
//                        name H W channels flags pyramid_tune n_levels <8 integers per level>
//                    (a name that starts with "null_levels" / "null_out" passes NULL for that pointer).  One line per plan: the status
//                    (and silent_last_error on a failure); the planner's decisions (class and trimmed zoom of every level, the stream
//                    path's layout, the walk's PX, plans and border pixels); a 64-bit hash (FNV-1a) of the TEXT of every scalar the
//                    plan carries and of every device pointer as its offset into the allocation it points to; size and hash of the
//                    bytes of the four table allocations; the per-launch decomposition of walk3_plan<float> on 1, 3 and 32 frames:
//                    tests/golden/plan_tables.txt
//   --text           the same with that text itself in place of its hash (about 1 KB per plan): run it on two builds and compare to
//                    see WHICH scalar moved
//   --alloc-faults   the same descriptions; each plan is created with silent_host_fail_new_after(k), k = 1, 2, ... until creation
//                    succeeds: every failing call returns SILENT_E_NOMEM and leaves *out NULL.  Run with LeakSanitizer ON: a plan or
//                    a table lost on such an exit is a leak report and a non-zero exit status.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <sanitizer/allocator_interface.h>

#ifndef SILENT_HOST_ONLY
#error "host-only build: compile with -DSILENT_HOST_ONLY (no GPU is touched)"
#endif
#include "../pysilent_amd/csrc/silent_unity.hip"

// ---- the plan's internals this driver reads (silent_plan.h): a member renamed there is an edit of these lines
struct PlanView {
    const silent::PyrTab& tab;
    const silent::PyrTab64& tab64;
    const std::vector<silent_extent>& extents;
    unsigned flags;
    bool f64;
    const float* unit_w;
    const double* unit_w64;
    bool stream_ok;
    int stream_layout, stream_unit_level;
    const silent::StreamTab& stream;
    bool walk_ok;
    int walk_px, walk_G;
    const silent::Walk3Args& walk;
    const silent::BorderTab& border;
    const void *tables, *tables64, *stream_tables, *walk_tables;
};
static PlanView view_of(const silent_pyramid_plan* p) {
    return PlanView{p->tab, p->tab64, p->extents, p->flags, p->f64, p->unit_w, p->unit_w64, p->stream_ok, p->stream_layout, p->stream_unit_level,
                    p->stream, p->walk_pyr_ok, p->walk_px, p->walk_G, p->walk, p->walk_border, p->tables, p->tables64, p->stream_tables,
                    p->walk_tables};
}
// ----

struct Case {
    std::string name;
    int H, W, channels, n_levels;
    unsigned flags, tune;
    std::vector<silent_pyr_level> levels;
};
static bool parse(const std::string& line, Case* c) {
    std::istringstream in(line);
    if (!(in >> c->name >> c->H >> c->W >> c->channels >> c->flags >> c->tune >> c->n_levels)) return false;
    int v[8];
    c->levels.clear();
    while (in >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6] >> v[7]) c->levels.push_back(silent_pyr_level{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]});
    if (c->levels.empty()) c->levels.push_back(silent_pyr_level{0, 0, 1, 1, 1, 1, 1, 1});     // (n_levels 0: a pointer that is not NULL)
    return true;
}
static int create(silent_ctx* ctx, const Case& c, silent_pyramid_plan** out) {
    const bool null_levels = c.name.rfind("null_levels", 0) == 0, null_out = c.name.rfind("null_out", 0) == 0;
    return silent_pyramid_plan_create_ex(ctx, c.H, c.W, c.channels, null_levels ? nullptr : c.levels.data(), c.n_levels, c.flags, null_out ? nullptr : out);
}

static std::string text;     // the line being built
static void put(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void put(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    text += buf;
}
static unsigned long long fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}
// size and hash of a whole allocation; a pointer into it as its offset
static void put_blob(const void* p) {
    if (!p) put(" | -");
    else put(" | %zu %016llx", __sanitizer_get_allocated_size(p), fnv(p, __sanitizer_get_allocated_size(p)));
}
static void put_off(const void* p, const void* base) {
    if (!p || !base) put(" -");
    else put(" %lld", (long long)((const char*)p - (const char*)base));
}
static bool same_scalars(const silent::PyrTab& a, const silent::PyrTab& b) {
    return a.n_levels == b.n_levels && a.H == b.H && a.W == b.W && a.C == b.C && a.frame_px_out == b.frame_px_out &&
           !std::memcmp(a.lv, b.lv, sizeof(a.lv)) && !std::memcmp(a.px_off, b.px_off, sizeof(a.px_off)) &&
           a.unit_tiles_per_frame == b.unit_tiles_per_frame && !std::memcmp(a.unit_tiles_x, b.unit_tiles_x, sizeof(a.unit_tiles_x)) &&
           !std::memcmp(a.unit_tile_start, b.unit_tile_start, sizeof(a.unit_tile_start)) && a.regions_x == b.regions_x && a.regions_y == b.regions_y &&
           a.n_general == b.n_general && a.zero_chunks_per_frame == b.zero_chunks_per_frame &&
           !std::memcmp(a.zero_chunk_start, b.zero_chunk_start, sizeof(a.zero_chunk_start)) && a.xidx == b.xidx && a.xw == b.xw && a.yidx == b.yidx &&
           a.yw == b.yw && a.xreg == b.xreg && a.yreg == b.yreg;
}

// the planner's decisions, short
static void decisions(const silent_pyramid_plan* plan) {
    const PlanView v = view_of(plan);
    put(" | lv");
    for (int l = 0; l < v.tab.n_levels; ++l) put(" %c%dx%d", v.tab.lv[l].kind == silent::kPyrUnit ? 'U' : 'G', v.tab.lv[l].zoom_h, v.tab.lv[l].zoom_w);
    put(" | stream %d layout %d unit %d G %d | walk %d px %d G %d plans %d border %d %d", (int)v.stream_ok, v.stream_layout, v.stream_unit_level, v.stream.G,
        (int)v.walk_ok, v.walk_px, v.walk_G, v.walk.n_plans, v.border.n, v.border.per_frame);
}
// every scalar and every pointer offset
static void scalars(const silent_pyramid_plan* plan) {
    const PlanView v = view_of(plan);
    const silent::PyrTab& t = v.tab;
    put(" | flags %u f64 %d ext", v.flags, (int)v.f64);
    for (const silent_extent& e : v.extents) put(" %dx%d", e.h, e.w);
    put(" | tab %d %d %d %d %lld tiles %d regions %d %d general %d zero %d", t.n_levels, t.H, t.W, t.C, t.frame_px_out, t.unit_tiles_per_frame, t.regions_x,
        t.regions_y, t.n_general, t.zero_chunks_per_frame);
    for (int l = 0; l < t.n_levels; ++l) {
        const silent::PyrLevelDev& d = t.lv[l];
        put(" | L%d %d  %d %d %d %d  %d %d %d %d  %d %d %d %d  %lld %d %d %d", l, d.kind, d.src_y0, d.src_x0, d.src_h, d.src_w, d.zoom_h, d.zoom_w, d.out_h, d.out_w,
            d.xtab_off, d.ytab_off, d.xreg_off, d.yreg_off, t.px_off[l], t.unit_tiles_x[l], t.unit_tile_start[l], t.zero_chunk_start[l]);
    }
    put(" | end %d %d", t.unit_tile_start[t.n_levels], t.zero_chunk_start[t.n_levels]);
    put(" | ptr");
    for (const void* p : {(const void*)t.xidx, (const void*)t.xw, (const void*)t.yidx, (const void*)t.yw, (const void*)t.xreg, (const void*)t.yreg}) put_off(p, v.tables);
    put(" | tab64 %s", same_scalars(v.tab64, t) ? "same" : same_scalars(v.tab64, silent::PyrTab{}) ? "unset" : "DIFFERENT");
    put_off(v.tab64.xw64, v.tables64);
    put_off(v.tab64.yw64, v.tables64);
    put(" | unit_w");
    for (int j = 0; j < 6; ++j) { uint32_t b; std::memcpy(&b, v.unit_w + j, 4); put(" %08x", b); }
    put(" | unit_w64");
    for (int j = 0; j < 6; ++j) { uint64_t b; std::memcpy(&b, v.unit_w64 + j, 8); put(" %016llx", (unsigned long long)b); }
    const silent::StreamTab& s = v.stream;
    put(" | stream %d layout %d unit %d G %d tiles_y %d waves_x %d px_off", (int)v.stream_ok, v.stream_layout, v.stream_unit_level, s.G, s.tiles_y, s.waves_x);
    for (int g = 0; g < 8; ++g) put(" %lld", s.px_off[g]);
    put(" out_w");
    for (int g = 0; g < 8; ++g) put(" %d", s.out_w[g]);
    put(" ptr");
    for (const int* p : {s.row_prog, s.col_hdr, s.col_rec}) put_off(p, v.stream_tables);
    const silent::Walk3Args& w = v.walk;
    put(" | walk %d px %d G %d  %d %d plans %d blocks %d frame_px %lld wx", (int)v.walk_ok, v.walk_px, v.walk_G, w.H, w.W, w.n_plans, w.blocks_per_frame, w.frame_px);
    for (int j = 0; j < 6; ++j) { uint32_t b; std::memcpy(&b, w.wx + j, 4); put(" %08x", b); }
    for (int pi = 0; pi < silent::kW3MaxPlans; ++pi) {
        const silent::Walk3Plan& p = w.plan[pi];
        static const silent::Walk3Plan none{};
        if (pi >= w.n_plans && !std::memcmp(&p, &none, sizeof(p))) continue;      // (an unused plan is printed where it is not all zero)
        put(" | P%d  %d %d %d %d shift %d unit %d  %d %d %d %d  %d %d %d %d  %lld G %d px_off", pi, p.src_y0, p.src_x0, p.src_h, p.src_w, p.shift, p.has_unit, p.out_h,
            p.out_w, p.eff_h, p.eff_w, p.strips_x, p.segs_y, p.seg_rows, p.block0, p.px_off, p.pyr.G);
        for (int g = 0; g < 8; ++g) put(" %lld", p.pyr.px_off[g]);
        put(" out_w");
        for (int g = 0; g < 8; ++g) put(" %d", p.pyr.out_w[g]);
        put(" ptr");
        for (const int* q : {p.pyr.row_prog, p.pyr.col_hdr, p.pyr.col_rec}) put_off(q, v.walk_tables);
    }
    const silent::BorderTab& b = v.border;
    put(" | border %d %d", b.n, b.per_frame);
    for (int i = 0; i < silent::kMaxLevels; ++i) {
        const silent::BorderLevel& l = b.lv[i];
        static const silent::BorderLevel none{};
        if (i >= b.n && !std::memcmp(&l, &none, sizeof(l))) continue;
        put(" | B%d %d  %d %d %d %d  %d %d %d", i, l.level, l.oy_lo, l.oy_hi, l.ox_lo, l.ox_hi, l.zr, l.zc, l.start);
    }
}
// the four allocations, and the per-launch decomposition (occupancy 5 and 256 CUs in this build, silent_host_shim.h)
static void tables_and_launches(silent_ctx* ctx, const silent_pyramid_plan* plan) {
    const PlanView v = view_of(plan);
    for (const void* p : {v.tables, v.tables64, v.stream_tables, v.walk_tables}) put_blob(p);    // (in this order)
    for (int n : {1, 3, 32}) {
        silent::Walk3Args wa;
        if (!v.walk_ok && n > 1 && !walk3_plan<float>(ctx, plan, n, &wa)) continue;     // (no walk: said once)
        if (!walk3_plan<float>(ctx, plan, n, &wa)) { put(" | launch%d -", n); continue; }
        put(" | launch%d blocks %d", n, wa.blocks_per_frame);
        for (int pi = 0; pi < wa.n_plans; ++pi) put("  %d %d %d %d", wa.plan[pi].strips_x, wa.plan[pi].seg_rows, wa.plan[pi].segs_y, wa.plan[pi].block0);
    }
}

static int tables(silent_ctx* ctx, bool as_text) {
    std::string line;
    Case c;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (!parse(line, &c)) { std::printf("cannot parse: %s\n", line.c_str()); return 2; }
        if (silent_set_tuning(ctx, SILENT_TUNE_PYRAMID, c.tune) != SILENT_OK) return 2;
        silent_pyramid_plan* plan = (silent_pyramid_plan*)(uintptr_t)8;      // (a failure must leave NULL here, where `out` is given)
        const int rc = create(ctx, c, &plan);
        text = c.name;
        put(" | %d", rc);
        if (rc != SILENT_OK) {
            put(" | %s | out %s", silent_last_error(ctx), plan == nullptr ? "NULL" : "untouched");
        } else {
            decisions(plan);
            const size_t at = text.size();
            scalars(plan);
            if (!as_text) {
                const unsigned long long h = fnv(text.data() + at, text.size() - at);
                text.resize(at);
                put(" | scalars %016llx", h);
            }
            tables_and_launches(ctx, plan);
            silent_pyramid_plan_destroy(plan);
        }
        std::printf("%s\n", text.c_str());
    }
    return 0;
}

static int alloc_faults(silent_ctx* ctx) {
    std::string line;
    Case c;
    int failures = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (!parse(line, &c)) { std::printf("cannot parse: %s\n", line.c_str()); return 2; }
        if (silent_set_tuning(ctx, SILENT_TUNE_PYRAMID, c.tune) != SILENT_OK) return 2;
        int k = 1, faults = 0;
        bool done = false;
        for (; k <= 400 && !done; ++k) {
            silent_pyramid_plan* plan = (silent_pyramid_plan*)(uintptr_t)8;
            silent_host_fail_new_after(k);           // (nothing of this program allocates between here and the reset)
            const int rc = create(ctx, c, &plan);
            silent_host_fail_new_after(0);
            if (rc == SILENT_OK) {
                silent_pyramid_plan_destroy(plan);
                done = true;
                break;
            }
            ++faults;
            if (rc != SILENT_E_NOMEM || plan != nullptr) {
                std::printf("%s: allocation %d failing -> status %d (%s), *out %s\n", c.name.c_str(), k, rc, silent_last_error(ctx), plan ? "not NULL" : "NULL");
                ++failures;
            }
        }
        if (!done) { std::printf("%s never succeeded within 400 allocations\n", c.name.c_str()); ++failures; }
        std::printf("%s | created with allocation %d failing no more | %d failures returned SILENT_E_NOMEM\n", c.name.c_str(), k, faults);
    }
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    silent_ctx* ctx = nullptr;
    if (silent_create(0, &ctx) != SILENT_OK) {
        std::printf("silent_create failed\n");
        return 2;
    }
    const int rc = argc > 1 && !std::strcmp(argv[1], "--alloc-faults") ? alloc_faults(ctx) : tables(ctx, argc > 1 && !std::strcmp(argv[1], "--text"));
    silent_destroy(ctx);
    if (rc == 2) std::printf("usage: [--text | --alloc-faults] < lines of: name H W channels flags pyramid_tune n_levels <8 integers per level>\n");
    return rc;
}
