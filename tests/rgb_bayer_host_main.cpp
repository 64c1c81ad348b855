// Stand-alone driver of silent_pyramid_bayer[_dev] and silent_bayer_to_rgb[_dev] (raw 8-bit Bayer mosaics for 3-channel plans) on the
// library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("rgb_bayer")).  ONE translation unit with silent_unity.hip,
// -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel launches are compiled out and device memory is host memory, so what
// runs is the argument validation, the plan tables, the host forms' staging and the walk loader's ADDRESS FUNCTION (w3_bayer_load,
// silent_walk_rgb.h: the function the kernel forms its addresses with) together with the integer half of its conversion
// (w3_bayer_sums: the columns a lane takes from its neighbours).
//   no argument     both forms of both entry points, for a classic and a crop plan, on mosaics in a heap block of EXACTLY the view's
//                   span for each layout (a staging size above the span reads past it: AddressSanitizer reports it; one below it leaves
//                   poison in the staging arena, which this program looks at); the status codes and the order of the checks; one "ok" line
//   --sizeof        sizeof(silent_bayer_frames) and the offset of every field, one line
//   --refusals      "name | case | status | silent_last_error" per (entry point, single fault)
//   --addresses LAYOUT H W n_levels <8 integers per level>
//                   every (block, chunk, row, lane, load slot) of the plan's walk launch on two frames: every offset is inside the span and
//                   is the byte of a pixel of the view, in a row in [0, H) that is yy - 1, yy or yy + 1 reflected; then the exchange of
//                   every ring row is replayed on a mosaic of random bytes -- lane j takes the packed column of lane j - 1 and j + 1
//                   across the load slots -- and for every pixel of the crop that the ring row holds, own sample and the three sums are
//                   those of the mosaic's 3 x 3 neighbourhood reflected at the frame's edges; every such pixel is written by some slot
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifndef SILENT_HOST_ONLY
#error "host-only build: compile with -DSILENT_HOST_ONLY (no GPU is touched)"
#endif
#include "../pysilent_amd/csrc/silent_unity.hip"

static int failures = 0;

#define EXPECT(call, want)                                                                                   \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != (want)) {                                                                                 \
            std::printf("line %d: %s -> %d, expected %d (%s)\n", __LINE__, #call, rc_, (int)(want), silent_last_error(ctx)); \
            ++failures;                                                                                      \
        }                                                                                                    \
    } while (0)

// a layout: the three strides and the offset of pixel (0, 0, 0) inside the buffer a camera or a caller would hold
struct Layout {
    long long ps, rs, fs, origin;
};
static bool layout_of(const char* name, int H, int W, Layout* l) {
    const std::string s(name);
    if (s == "packed") *l = Layout{1, W, (long long)H * W, 0};
    else if (s == "pitched") *l = Layout{1, W + 13, (long long)H * (W + 13) + 57, 0};
    else if (s == "pixel_stride_2") *l = Layout{2, 2 * W + 7, (long long)H * (2 * W + 7) + 31, 0};
    else if (s == "odd_window") *l = Layout{1, W + 12, (long long)(H + 9) * (W + 12), 3 * (W + 12) + 5};   // row 3, column 5 of larger images
    else return false;
    return true;
}
static long long span_of(const Layout& l, int n, int H, int W) { return (n - 1) * l.fs + (long long)(H - 1) * l.rs + (long long)(W - 1) * l.ps + 1; }
static silent_bayer_frames frames_of(const uint8_t* data, const Layout& l, int pattern, int order) {
    silent_bayer_frames f;
    f.data = data;
    f.pixel_stride = l.ps;
    f.row_stride = l.rs;
    f.frame_stride = l.fs;
    f.pattern = pattern;
    f.order = order;
    return f;
}
static int reflect(int i, int n) { return i < 0 ? -i : (i > n - 1 ? 2 * (n - 1) - i : i); }
static int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct Args {
    silent_ctx* ctx; const silent_pyramid_plan* plan; silent_bayer_frames f; const silent_bayer_frames* fp; int n, H, W; float* out;
};
static const char* const kFaultNames[] = {"plan NULL", "struct NULL", "data NULL", "pattern 4", "pattern -1", "order 2", "order -1", "H 1", "W 1",
                                          "pixel_stride 0", "pixel_stride -1", "row_stride 0", "row_stride below its row extent",
                                          "frame_stride below its bound", "frame_stride 0", "frame_stride -1", "span of 2^63 bytes", "out NULL",
                                          "plan of another context", "n_frames 0", "n_frames -1", "single-channel plan", "float64 plan"};
static void refusal_table(const Args& valid, const silent_pyramid_plan* plan_h1, const silent_pyramid_plan* plan_w1, const silent_pyramid_plan* plan_other,
                          const silent_pyramid_plan* plan_gray, const silent_pyramid_plan* plan_f64) {
    const int n_faults = (int)(sizeof(kFaultNames) / sizeof(kFaultNames[0]));
    const char* const names[4] = {"silent_pyramid_bayer", "silent_pyramid_bayer_dev", "silent_bayer_to_rgb", "silent_bayer_to_rgb_dev"};
    for (int e = 0; e < 4; ++e)
        for (int k = 0; k < n_faults; ++k) {
            const bool pyramid = e < 2;
            if (!pyramid && (k == 0 || k == 18 || k == 21 || k == 22)) continue;      // (no plan argument)
            Args a = valid;
            a.fp = &a.f;
            switch (k) {
                case 0: a.plan = nullptr; break;
                case 1: a.fp = nullptr; break;
                case 2: a.f.data = nullptr; break;
                case 3: a.f.pattern = 4; break;
                case 4: a.f.pattern = -1; break;
                case 5: a.f.order = 2; break;
                case 6: a.f.order = -1; break;
                case 7: a.plan = plan_h1; a.H = 1; break;
                case 8: a.plan = plan_w1; a.W = 1; break;
                case 9: a.f.pixel_stride = 0; break;
                case 10: a.f.pixel_stride = -1; break;
                case 11: a.f.row_stride = 0; break;
                case 12: a.f.row_stride = (valid.W - 1) * a.f.pixel_stride; break;
                case 13: a.f.frame_stride = (valid.H - 1) * a.f.row_stride + (valid.W - 1) * a.f.pixel_stride; break;
                case 14: a.f.frame_stride = 0; break;
                case 15: a.f.frame_stride = -1; break;
                case 16: a.f.frame_stride = 1ll << 62; a.n = 3; break;
                case 17: a.out = nullptr; break;
                case 18: a.plan = plan_other; break;
                case 19: a.n = 0; break;
                case 20: a.n = -1; break;
                case 21: a.plan = plan_gray; break;
                case 22: a.plan = plan_f64; break;
            }
            int rc;
            if (e == 0) rc = silent_pyramid_bayer(a.ctx, a.plan, a.fp, a.n, a.out);
            else if (e == 1) rc = silent_pyramid_bayer_dev(a.ctx, a.plan, a.fp, a.n, a.out, nullptr);
            else if (e == 2) rc = silent_bayer_to_rgb(a.ctx, a.fp, a.n, a.H, a.W, a.out);
            else rc = silent_bayer_to_rgb_dev(a.ctx, a.fp, a.n, a.H, a.W, a.out, nullptr);
            std::printf("%s | %s | %d | %s\n", names[e], kFaultNames[k], rc, rc == SILENT_OK ? "-" : silent_last_error(a.ctx));
        }
}

// ---- --addresses
static int addresses(silent_ctx* ctx, int argc, char** argv) {
    if (argc < 6) return 2;
    const int H = std::atoi(argv[3]), W = std::atoi(argv[4]), nl = std::atoi(argv[5]), n = 2;
    Layout lay;
    if (!layout_of(argv[2], H, W, &lay) || argc != 6 + 8 * nl) return 2;
    std::vector<silent_pyr_level> levels(nl);
    for (int l = 0; l < nl; ++l) {
        int v[8];
        for (int i = 0; i < 8; ++i) v[i] = std::atoi(argv[6 + 8 * l + i]);
        levels[l] = silent_pyr_level{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    }
    silent_pyramid_plan* plan = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, levels.data(), nl, &plan), SILENT_OK);
    if (failures) return 1;
    silent::Walk3Args wa;
    if (!walk3_plan<Bayer>(ctx, plan, n, &wa)) {
        std::printf("%d x %d: the plan has no walk launch\n", H, W);
        return 1;
    }
    const int px = plan->walk_px, loads = silent::w3_bayer_row_loads(px), slots = 64 * loads, row_f = silent::w3_row_f(px);
    const long long span = span_of(lay, n, H, W);
    // the mosaic: random bytes at the pixels of the view, in a block of exactly the span (data at address 0 for the offsets)
    std::vector<uint8_t> bytes((size_t)span, 0), is_pixel((size_t)span, 0), touched((size_t)span, 0);
    unsigned rnd = 12345u;
    for (int f = 0; f < n; ++f)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t o = (size_t)(f * lay.fs + y * lay.rs + x * lay.ps);
                rnd = rnd * 1664525u + 1013904223u;
                bytes[o] = (uint8_t)(rnd >> 24);
                is_pixel[o] = 1;
            }
    auto m = [&](int f, int y, int x) { return (int)bytes[(size_t)(f * lay.fs + reflect(y, H) * lay.rs + reflect(x, W) * lay.ps)]; };
    const Bayer v{nullptr, lay.ps, lay.rs, lay.fs, H, W, 0, 0};
    long long n_loads = 0, outside = 0, not_pixel = 0, wrong_row = 0, wrong_offset = 0, checked = 0, wrong_sums = 0, unwritten = 0;
    std::vector<int> pk((size_t)slots), col((size_t)slots);
    std::vector<uint8_t> done;
    for (unsigned bid = 0; bid < (unsigned)(n * wa.blocks_per_frame); ++bid) {
        const silent::W3ViewBlock b = silent::w3_view_block(wa, px, bid);
        const silent::Walk3Plan& w = wa.plan[b.plan];
        for (int c = 0; c < b.n_chunks; ++c)
            for (int r = 0; r < silent::kW3CH; ++r) {
                int yy = -1;
                for (int k = 0; k < loads; ++k)
                    for (int lane = 0; lane < 64; ++lane) {
                        const silent::W3BayerLoad L = silent::w3_bayer_load(wa, v, px, bid, c, r, lane, k);
                        int e[3] = {0, 0, 0};
                        yy = L.row[1];
                        if (L.row[1] < 0 || L.row[1] >= H || L.row[0] != reflect(L.row[1] - 1, H) || L.row[2] != reflect(L.row[1] + 1, H) || L.col < 0 || L.col >= W)
                            ++wrong_row;
                        for (int i = 0; i < 3; ++i) {
                            ++n_loads;
                            if (L.offset[i] < 0 || L.offset[i] + 1 > span) {
                                if (!outside++) std::printf("block %u chunk %d row %d lane %d slot %d: offset %lld of %lld\n", bid, c, r, lane, k, L.offset[i], span);
                                continue;
                            }
                            if (L.offset[i] != b.frame * lay.fs + L.row[i] * lay.rs + L.col * lay.ps) ++wrong_offset;
                            if (!is_pixel[(size_t)L.offset[i]]) ++not_pixel;
                            touched[(size_t)L.offset[i]] = 1;
                            e[i] = bytes[(size_t)L.offset[i]];
                        }
                        pk[(size_t)(64 * k + lane)] = e[0] | (e[1] << 8) | (e[2] << 16);
                        col[(size_t)(64 * k + lane)] = L.col;
                    }
                if (outside) continue;
                // the exchange and the sums, for the pixels of the crop this ring row holds
                done.assign((size_t)W, 0);
                for (int j = 0; j < slots; ++j) {
                    const int p = silent::w3_bayer_p0(b.A) + j, q = silent::w3_bayer_ring_float(b.A, j & 63, j >> 6);
                    if (q < 0 || q + 2 >= row_f || p < w.src_x0 || p >= w.src_x0 + w.src_w) continue;     // not a whole pixel of the crop in the ring
                    const silent::W3BayerSums s = silent::w3_bayer_sums(W, j > 0 ? pk[(size_t)(j - 1)] : 0, pk[(size_t)j], j + 1 < slots ? pk[(size_t)(j + 1)] : 0, col[(size_t)j]);
                    ++checked;
                    const int f = b.frame;
                    const bool ok = col[(size_t)j] == p && s.c == m(f, yy, p) && s.h == m(f, yy, p - 1) + m(f, yy, p + 1) && s.v == m(f, yy - 1, p) + m(f, yy + 1, p) &&
                                    s.d == m(f, yy - 1, p - 1) + m(f, yy - 1, p + 1) + m(f, yy + 1, p - 1) + m(f, yy + 1, p + 1);
                    if (!ok && !wrong_sums++) std::printf("block %u chunk %d row %d slot %d: pixel (%d, %d) of frame %d gets other samples\n", bid, c, r, j, yy, p, f);
                    done[(size_t)p] = 1;
                }
                // every pixel of the crop between the ring row's first and last whole pixel is written
                // (ring float i holds float A + i of the virtual packed frame row: pixel p is whole in it for A <= 3 p and 3 p + 2 < A + row_f)
                const int lo_ring = floor_div(b.A + 2, 3), hi_ring = floor_div(b.A + row_f - 3, 3) + 1;
                const int lo = lo_ring > w.src_x0 ? lo_ring : w.src_x0, hi = hi_ring < w.src_x0 + w.src_w ? hi_ring : w.src_x0 + w.src_w;
                for (int p = lo; p < hi; ++p) unwritten += !done[(size_t)p];
            }
    }
    // the 3 x 3 neighbourhood (reflected) of every pixel of every walk plan's crop was fetched by someone
    long long needed = 0, missing = 0;
    int odd_origin = 0;
    for (int p = 0; p < wa.n_plans; ++p) odd_origin += (wa.plan[p].src_x0 & 1) && (wa.plan[p].src_y0 & 1);
    for (int f = 0; f < n; ++f)
        for (int p = 0; p < wa.n_plans; ++p) {
            const silent::Walk3Plan& w = wa.plan[p];
            for (int y = w.src_y0; y < w.src_y0 + w.src_h; ++y)
                for (int x = w.src_x0; x < w.src_x0 + w.src_w; ++x)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            ++needed;
                            missing += !touched[(size_t)(f * lay.fs + reflect(y + dy, H) * lay.rs + reflect(x + dx, W) * lay.ps)];
                        }
        }
    std::printf("%s %d x %d | plans %d px %d blocks %d | loads %lld | outside %lld | not a pixel byte %lld | wrong rows %lld offsets %lld | pixels checked %lld "
                "wrong sums %lld unwritten %lld | needed %lld missing %lld | odd origins %d\n",
                argv[2], H, W, wa.n_plans, px, n * wa.blocks_per_frame, n_loads, outside, not_pixel, wrong_row, wrong_offset, checked, wrong_sums, unwritten, needed,
                missing, odd_origin);
    if (outside || not_pixel || wrong_row || wrong_offset || wrong_sums || unwritten || missing || !needed || !checked) ++failures;
    silent_pyramid_plan_destroy(plan);
    return failures ? 1 : 0;
}

// the host form stages exactly the view's span at arena offset 0, the output behind it on the following multiple of 256; the arena is
// poisoned, the call made, the bytes compared and the poison behind the span looked at
template <class Call>
static void check_arena(silent_ctx* ctx, const char* what, const uint8_t* data, size_t span, size_t out_bytes, Call&& call) {
    const size_t out_at = (span + 255) / 256 * 256;
    if (!ctx->arena.p || ctx->arena.cap < out_at + out_bytes) {
        std::printf("%s: the staging arena holds %zu bytes, expected at least %zu\n", what, (size_t)ctx->arena.cap, out_at + out_bytes);
        ++failures;
        return;
    }
    std::memset(ctx->arena.p, 0xEE, ctx->arena.cap);
    EXPECT(call(), SILENT_OK);
    const uint8_t* arena = (const uint8_t*)ctx->arena.p;
    if (std::memcmp(arena, data, span) != 0) { std::printf("%s: the staged bytes differ\n", what); ++failures; }
    if (span % 256 == 0) { std::printf("%s: the span is a multiple of 256\n", what); ++failures; }
    for (size_t b = span; b < out_at; ++b)
        if (arena[b] != 0xEE) { std::printf("%s: byte %zu of the arena was written: more than %zu bytes were staged\n", what, b, span); ++failures; break; }
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
    const int H = 41, W = 59, n = 2;          // odd extents
    if (argc > 1 && !std::strcmp(argv[1], "--sizeof")) {
        std::printf("sizeof %zu | data %zu pixel_stride %zu row_stride %zu frame_stride %zu pattern %zu order %zu\n", sizeof(silent_bayer_frames),
                    offsetof(silent_bayer_frames, data), offsetof(silent_bayer_frames, pixel_stride), offsetof(silent_bayer_frames, row_stride),
                    offsetof(silent_bayer_frames, frame_stride), offsetof(silent_bayer_frames, pattern), offsetof(silent_bayer_frames, order));
        return 0;
    }
    silent_ctx* ctx = nullptr;
    silent_ctx* other = nullptr;
    if (silent_create(0, &ctx) != SILENT_OK || silent_create(0, &other) != SILENT_OK) {
        std::printf("silent_create failed\n");
        return 2;
    }
    if (argc > 1 && !std::strcmp(argv[1], "--addresses")) {
        const int rc = addresses(ctx, argc, argv);
        silent_destroy(other);
        silent_destroy(ctx);
        if (rc == 2) std::printf("usage: --addresses LAYOUT H W n_levels <8 integers per level>\n");
        return rc;
    }
    const silent_pyr_level ladder[3] = {{0, 0, H, W, H, W, H, W}, {0, 0, H, W, 20, 29, 20, 29}, {0, 0, H, W, 10, 14, 10, 14}};
    const silent_pyr_level crops[3] = {{3, 5, 30, 41, 30, 41, 30, 41}, {0, 0, H, W, 20, 29, 22, 31}, {11, 17, 20, 33, 10, 17, 10, 17}};
    const silent_pyr_level ladder_h1[1] = {{0, 0, 1, W, 1, W, 1, W}}, ladder_w1[1] = {{0, 0, H, 1, H, 1, H, 1}};
    silent_pyramid_plan *plan = nullptr, *plan_crop = nullptr, *plan_gray = nullptr, *plan_f64 = nullptr, *plan_other = nullptr, *plan_h1 = nullptr, *plan_w1 = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, ladder, 3, &plan), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, crops, 3, &plan_crop), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, ladder, 3, &plan_gray), SILENT_OK);
    EXPECT(silent_pyramid_plan_create_ex(ctx, H, W, 1, ladder, 3, SILENT_PLAN_ACCUM_F64, &plan_f64), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(other, H, W, 3, ladder, 3, &plan_other), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, 1, W, 3, ladder_h1, 1, &plan_h1), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, 1, 3, ladder_w1, 1, &plan_w1), SILENT_OK);
    if (failures) return 1;

    const char* const kinds[4] = {"packed", "pitched", "pixel_stride_2", "odd_window"};
    std::vector<float> rgb((size_t)n * H * W * 3);
    for (int kind = 0; kind < 4; ++kind) {
        Layout lay;
        layout_of(kinds[kind], H, W, &lay);
        const size_t span = (size_t)span_of(lay, n, H, W);
        uint8_t* block = (uint8_t*)std::malloc(span);              // EXACTLY the span: the window's origin is the block's first byte
        for (size_t i = 0; i < span; ++i) block[i] = (uint8_t)(i * 37 + 11);
        const silent_bayer_frames fr = frames_of(block, lay, kind, kind & 1);
        const silent_pyramid_plan* plans[2] = {plan, plan_crop};
        for (const silent_pyramid_plan* p : plans) {
            const size_t px = (size_t)n * (p == plan ? 41 * 59 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
            std::vector<float> pyr(px * 3);
            if (refusals) {
                if (p == plan && kind == 1) refusal_table(Args{ctx, p, fr, nullptr, n, H, W, pyr.data()}, plan_h1, plan_w1, plan_other, plan_gray, plan_f64);
                continue;
            }
            EXPECT(silent_pyramid_bayer(ctx, p, &fr, n, pyr.data()), SILENT_OK);
            EXPECT(silent_pyramid_bayer_dev(ctx, p, &fr, n, pyr.data(), nullptr), SILENT_OK);
            EXPECT(silent_bayer_to_rgb(ctx, &fr, n, H, W, rgb.data()), SILENT_OK);
            EXPECT(silent_bayer_to_rgb_dev(ctx, &fr, n, H, W, rgb.data(), nullptr), SILENT_OK);
            check_arena(ctx, kinds[kind], block, span, pyr.size() * 4, [&] { return silent_pyramid_bayer(ctx, p, &fr, n, pyr.data()); });
            check_arena(ctx, kinds[kind], block, span, rgb.size() * 4, [&] { return silent_bayer_to_rgb(ctx, &fr, n, H, W, rgb.data()); });
            if (kind != 1) continue;
            // one frame: the frame stride is not read (a block of exactly the one-frame span)
            {
                const size_t span1 = (size_t)span_of(lay, 1, H, W);
                uint8_t* a = (uint8_t*)std::malloc(span1);
                std::memset(a, 90, span1);
                silent_bayer_frames one = frames_of(a, lay, 2, 1);
                one.frame_stride = -5;
                EXPECT(silent_pyramid_bayer(ctx, p, &one, 1, pyr.data()), SILENT_OK);
                EXPECT(silent_pyramid_bayer_dev(ctx, p, &one, 1, pyr.data(), nullptr), SILENT_OK);
                EXPECT(silent_bayer_to_rgb(ctx, &one, 1, H, W, rgb.data()), SILENT_OK);
                std::free(a);
            }
            // the smallest frames: 2 x 2 and 3 x 2, in blocks of exactly their spans
            for (int hh = 2; hh <= 3; ++hh) {
                const Layout l2{1, 2, (long long)hh * 2, 0};
                uint8_t* a = (uint8_t*)std::malloc((size_t)span_of(l2, n, hh, 2));
                std::memset(a, 7, (size_t)span_of(l2, n, hh, 2));
                const silent_bayer_frames f2 = frames_of(a, l2, 3, 0);
                EXPECT(silent_bayer_to_rgb(ctx, &f2, n, hh, 2, rgb.data()), SILENT_OK);
                std::free(a);
            }
            // ---- status codes and the order of the checks: a NULL ctx before everything; the struct's own refusals in the header's
            // order and before the shared checks; NULL before the context, the context before n_frames, n_frames before the plan's kind
            silent_bayer_frames bad = fr;
            EXPECT(silent_pyramid_bayer(nullptr, nullptr, nullptr, 0, nullptr), SILENT_E_INVALID);
            EXPECT(silent_bayer_to_rgb_dev(nullptr, nullptr, 0, 0, 0, nullptr, nullptr), SILENT_E_INVALID);
            EXPECT(silent_pyramid_bayer(ctx, plan_gray, &fr, n, pyr.data()), SILENT_E_UNSUPPORTED);
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_gray, &fr, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
            if (!std::strstr(silent_last_error(ctx), "3-channel plans")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_f64, &fr, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
            bad.row_stride = 3;
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "row_stride")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.pixel_stride = 0;                                     // the pixel stride before the row stride
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "pixel_stride")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.order = 7;                                            // the order before a stride
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "order must be")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.pattern = 4;                                          // the pattern before the order
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "pattern must be")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_bayer(ctx, plan_other, &fr, 0, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "NULL pointer")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_bayer_dev(ctx, plan_other, &fr, 0, pyr.data(), nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "another context")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_bayer(ctx, plan_gray, &fr, 0, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "n_frames")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_bayer_to_rgb(ctx, &fr, n, 1, W, rgb.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "at least 2")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
            // the float32 call still takes what it took
            EXPECT(silent_pyramid(ctx, p, rgb.data(), n, pyr.data()), SILENT_OK);
        }
        std::free(block);
    }
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    for (silent_pyramid_plan* q : {plan, plan_crop, plan_gray, plan_f64, plan_other, plan_h1, plan_w1}) silent_pyramid_plan_destroy(q);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    if (!refusals) std::printf("rgb bayer host main ok\n");
    return 0;
}
