// Stand-alone driver of the attention tail's host side (silent_attention_tail[_dev], silent_attention_extents; the planning:
// pysilent_amd/csrc/silent_peaks_plan.h, attention_plan) on the library's HOST side (pysilent_amd/csrc/build.py,
// build_host_driver("attn_tables")).  ONE translation unit with silent_unity.hip, -DSILENT_HOST_ONLY, under -fsanitize=address,undefined;
// launches are compiled out.  Case lines on stdin:
//     name n_frames rh rw resize_div recovery_mode visualize want n_levels <h w per level>
// want: bit 0 centroids_out, bit 1 centroids2_out, bit 2 fired_out, bit 3 update_out.  A name that starts with null_value / null_energy /
// null_params / null_levels passes NULL there.
//   no argument   every case runs silent_attention_tail_dev on a fresh context (buffers of one float: nothing is launched) and prints the
//                 status (and silent_last_error on a refusal); an accepted case then prints what attention_plan built -- per level the
//                 three extents silent_attention_extents gives, the SAME-padding firsts and float32 scales of both cell tables, the resize
//                 scales, the tile starts of the three index spaces -- the block counts, the cell totals, every piece of the workspace as
//                 an offset, its total and the context's capacity.
//   --layout      attention_plan alone (pure: sizes nobody wants to allocate under a sanitizer), one "ok" line per case.
// Every accepted case is CHECKED here, with this file's own arithmetic: the pieces are 256-aligned, pairwise disjoint, inside the total
// and hold 8 + 8 + 4 + 4 bytes per cell; the block counts are those of 64 x 64 tiles and 1024-cell chunks; the kernel's block ranges
// b1 / b2 are their prefix sums; what silent_attention_extents returns is what the plan holds -- exit status 1 otherwise.
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

struct Case {
    std::string name;
    int n_frames, rh, rw, mode, visualize, want, n_levels;
    float div;
    std::vector<silent_extent> levels;
};
static bool parse(const std::string& line, Case* c) {
    std::istringstream in(line);
    std::string div;
    if (!(in >> c->name >> c->n_frames >> c->rh >> c->rw >> div >> c->mode >> c->visualize >> c->want >> c->n_levels)) return false;
    c->div = div == "nan" ? NAN : div == "inf" ? INFINITY : (float)std::atof(div.c_str());
    c->levels.clear();
    int h, w;
    while (in >> h >> w) c->levels.push_back(silent_extent{h, w});
    if (c->levels.empty()) c->levels.push_back(silent_extent{1, 1});   // (n_levels 0: a pointer that is not NULL)
    return true;
}
static bool starts(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }
static unsigned bits(float f) {
    unsigned b;
    std::memcpy(&b, &f, 4);
    return b;
}
static silent_attention_params params_of(const Case& c) {
    silent_attention_params p;
    std::memset(&p, 0, sizeof(p));
    p.region_h = c.rh;
    p.region_w = c.rw;
    p.resize_div = c.div;
    p.boosting.exhaustion_max = p.boosting.excitation_max = 1.0f;
    p.boosting.recovery_mode = (unsigned)c.mode;
    p.boosting.recovery_amount = 10.0f;
    p.boosting.recovery_percentage = 0.8f;
    p.boosting.visualize = c.visualize;
    return p;
}

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }
static long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// what must hold of an accepted plan
static bool check_plan(const Case& c, const silent::AttnPlan& ap) {
    bool ok = true;
    auto bad = [&](const char* what) {
        std::printf("CHECK FAILED %s: %s\n", c.name.c_str(), what);
        ok = false;
    };
    const bool dist = c.want & 1, half = c.want & 2;
    long long cells = 0, cells2 = 0, t1 = 0, t2 = 0, tc = 0;
    for (int l = 0; l < c.n_levels; ++l) {
        const long long ch = ceil_div(c.levels[l].h, c.rh), cw = ceil_div(c.levels[l].w, c.rw);
        const long long ch2 = ceil_div(ap.half[l].h, c.rh), cw2 = ceil_div(ap.half[l].w, c.rw);
        cells += ch * cw;
        cells2 += ch2 * cw2;
        t1 += ceil_div(c.levels[l].h, 64) * ceil_div(c.levels[l].w, 64);
        t2 += ceil_div(ap.half[l].h, 64) * ceil_div(ap.half[l].w, 64);
        tc += ceil_div(ch * cw, 1024);
        if (ap.cells[l].h != ch || ap.cells[l].w != cw || ap.cells2[l].h != ch2 || ap.cells2[l].w != cw2) bad("cell extents");
    }
    const long long nf = c.n_frames;
    if (ap.n_cells != cells * nf || ap.n_cells2 != (half ? cells2 * nf : 0)) bad("cell totals");
    if (ap.px_blocks != (dist ? t1 * nf : 0) || ap.px2_blocks != (half ? t2 * nf : 0) || ap.cell_blocks != tc * nf) bad("block counts");
    if (ap.t.b1 != (unsigned)ap.px_blocks || ap.t.b2 != (unsigned)(ap.px_blocks + ap.px2_blocks)) bad("block ranges of the pixel kernel");
    if (ap.t.n_cells != ap.n_cells || ap.t.n_cells2 != ap.n_cells2 || ap.t.n_frames != c.n_frames) bad("totals in the kernel argument");
    struct Piece { const char* name; size_t off, bytes; };
    const Piece p[4] = {{"cxy", ap.ws.cxy, (size_t)ap.n_cells * 8}, {"cxy2", ap.ws.cxy2, (size_t)ap.n_cells2 * 8},
                        {"imp", ap.ws.imp, (size_t)ap.n_cells * 4}, {"m", ap.ws.m, (size_t)ap.n_cells * 4}};
    size_t sum = 0;
    for (int i = 0; i < 4; ++i) {
        if (p[i].off % 256) bad("a piece is not 256-aligned");
        if (p[i].off + p[i].bytes > ap.ws.total) bad("a piece ends outside the total");
        for (int j = 0; j < i; ++j)
            if (p[i].bytes && p[j].bytes && p[i].off < p[j].off + p[j].bytes && p[j].off < p[i].off + p[i].bytes) bad("two pieces overlap");
        sum += up256(p[i].bytes);
    }
    if (sum != ap.ws.total) bad("the total is not the sum of the pieces (8 + 8 + 4 + 4 bytes per cell, each rounded up to 256)");
    return ok;
}

static void print_plan(const Case& c, const silent::AttnPlan& ap, size_t cap) {
    for (int l = 0; l < c.n_levels; ++l) {
        const silent::AttnTab& t = ap.t;
        std::printf("%s L%d | cells %d %d half %d %d cells2 %d %d | first %d %d %d %d | scale %08x %08x %08x %08x | resize %08x %08x | "
                    "tiles %d %d %d | off %lld %lld %lld %lld\n",
                    c.name.c_str(), l, ap.cells[l].h, ap.cells[l].w, ap.half[l].h, ap.half[l].w, ap.cells2[l].h, ap.cells2[l].w, t.ct1.y_first[l],
                    t.ct1.x_first[l], t.ct2.y_first[l], t.ct2.x_first[l], bits(t.ct1.yscale[l]), bits(t.ct1.xscale[l]), bits(t.ct2.yscale[l]),
                    bits(t.ct2.xscale[l]), bits(t.yscale_r[l]), bits(t.xscale_r[l]), t.tab1.tile_start[l], t.tab2.tile_start[l], t.tabc.tile_start[l],
                    t.tab1.px_off[l], t.tab2.px_off[l], t.ct1.cell_off[l], t.ct2.cell_off[l]);
    }
    std::printf("%s plan | blocks %lld %lld %lld | cells %lld %lld | px %lld %lld | ws cxy %zu cxy2 %zu imp %zu m %zu total %zu | cap %zu | visualize %d\n",
                c.name.c_str(), ap.px_blocks, ap.px2_blocks, ap.cell_blocks, ap.n_cells, ap.n_cells2, ap.frame_px, ap.frame_px2, ap.ws.cxy, ap.ws.cxy2,
                ap.ws.imp, ap.ws.m, ap.ws.total, cap, ap.t.bp.visualize);
}

static bool tables_case(const Case& c) {
    silent_ctx* ctx = nullptr;
    if (silent_create(0, &ctx) != SILENT_OK) return false;
    bool ok = true;
    silent_attention_params p = params_of(c);
    float one[6] = {0, 0, 0, 0, 0, 0};
    const silent_extent* levels = starts(c.name, "null_levels") ? nullptr : c.levels.data();
    const int rc = silent_attention_tail_dev(ctx, starts(c.name, "null_value") ? nullptr : &one[0], levels, c.n_levels, c.n_frames,
                                             starts(c.name, "null_params") ? nullptr : &p, starts(c.name, "null_energy") ? nullptr : &one[1],
                                             c.want & 1 ? &one[2] : nullptr, c.want & 2 ? &one[3] : nullptr, c.want & 4 ? &one[4] : nullptr,
                                             c.want & 8 ? &one[5] : nullptr, nullptr);
    if (rc != SILENT_OK) {
        std::printf("%s | %d | %s\n", c.name.c_str(), rc, silent_last_error(ctx));
    } else {
        std::printf("%s | 0\n", c.name.c_str());
        silent::AttnPlan ap;
        const silent::Refusal r = silent::attention_plan(c.levels.data(), c.n_levels, c.n_frames, &p, c.want & 1, c.want & 2, &ap);
        if (r.status != SILENT_OK) {
            std::printf("CHECK FAILED %s: the entry point accepted what attention_plan refuses\n", c.name.c_str());
            ok = false;
        } else {
            print_plan(c, ap, ctx->ws.cap);
            ok = check_plan(c, ap);
            if (ctx->ws.cap < ap.ws.total) {
                std::printf("CHECK FAILED %s: the context's workspace is smaller than the layout's total\n", c.name.c_str());
                ok = false;
            }
            std::vector<silent_extent> a(c.n_levels), b(c.n_levels), d(c.n_levels);
            if (silent_attention_extents(c.levels.data(), c.n_levels, &p, a.data(), b.data(), d.data()) != SILENT_OK ||
                std::memcmp(a.data(), ap.cells, sizeof(silent_extent) * c.n_levels) || std::memcmp(b.data(), ap.half, sizeof(silent_extent) * c.n_levels) ||
                std::memcmp(d.data(), ap.cells2, sizeof(silent_extent) * c.n_levels)) {
                std::printf("CHECK FAILED %s: silent_attention_extents and the plan disagree\n", c.name.c_str());
                ok = false;
            }
        }
    }
    silent_destroy(ctx);
    return ok;
}

static bool layout_case(const Case& c) {
    silent_attention_params p = params_of(c);
    silent::AttnPlan ap;
    const silent::Refusal r = silent::attention_plan(c.levels.data(), c.n_levels, c.n_frames, &p, c.want & 1, c.want & 2, &ap);
    if (r.status != SILENT_OK) {
        std::printf("%s layout | %d | %s\n", c.name.c_str(), r.status, r.tail);
        return false;
    }
    if (!check_plan(c, ap)) return false;
    std::printf("%s layout | ok | cells %lld %lld blocks %lld %lld %lld total %zu\n", c.name.c_str(), ap.n_cells, ap.n_cells2, ap.px_blocks, ap.px2_blocks,
                ap.cell_blocks, ap.ws.total);
    return true;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (!mode.empty() && mode != "--layout") {
        std::printf("usage: [--layout] < case lines (see the head of tests/attention_tail_host_main.cpp)\n");
        return 2;
    }
    int rc = 0;
    std::string line;
    Case c;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (!parse(line, &c)) return 2;
        if (!(mode.empty() ? tables_case(c) : layout_case(c))) rc = 1;
    }
    return rc;
}
