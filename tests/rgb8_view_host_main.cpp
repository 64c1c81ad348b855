// Stand-alone driver of silent_pyramid_rgb8_view / silent_pyramid_rgb8_view_dev (strided uint8 colour views for 3-channel plans) on the
// library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("rgb8_view")).  ONE translation unit with silent_unity.hip,
// -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel launches are compiled out and device memory is host memory, so what
// runs is the argument validation, the plan tables, the host form's staging and the walk loader's ADDRESS FUNCTION (w3_view_load,
// silent_walk_rgb.h: the function the kernel forms its addresses with).
//   no argument     both forms on views whose data is a heap block of EXACTLY `span` bytes (a staging size above span reads past it:
//                   AddressSanitizer reports it; one below it leaves poison in the staging arena, which this program looks at), the
//                   status codes and the order of the checks; one "ok" line
//   --refusals      "name | case | status | silent_last_error" per (entry point, single fault): tests/golden/rgb8_view_refusals.txt
//   --addresses H W n_levels <8 integers per level>
//                   every (block, chunk, row, lane, load slot) of the plan's walk launch on two frames, for each kind of view:
//                   every access inside [0, span), every access wider than a byte aligned to its width, and the union of the bytes
//                   touched contains every channel byte of every pixel of every walk plan's crop; one line per view kind
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// the kinds of view of tests/rgb_strided_views.py as (offset of pixel (0, 0, 0) in its parent, pixel, row, frame stride)
struct Kind {
    const char* name;
    long long offset, pixel, row, frame;
};
static std::vector<Kind> kinds(int H, int W) {
    const long long h = H, w = W;
    return {{"bgra", 0, 4, 4 * w, 4 * w * h},
            {"bgra at byte 1", 1, 4, 4 * w, 4 * w * h},
            {"odd-pitch bgr", 0, 3, 3 * w + 5, (3 * w + 5) * h},
            {"region at (7, 5)", (7 * (w + 13) + 5) * 3, 3, (w + 13) * 3, (h + 20) * (w + 13) * 3},
            {"every second pixel", 0, 6, 6 * w, 6 * w * h},
            {"frames with a gap", 3, 3, 3 * w, 3 * w * h + 1001}};
}
static long long span_of(const Kind& k, int n, int H, int W) {
    return (long long)(n - 1) * k.frame + (long long)(H - 1) * k.row + (long long)(W - 1) * k.pixel + 3;
}

struct Args {
    silent_ctx* ctx; const silent_pyramid_plan* plan; silent_frame_view view; const silent_frame_view* vp; int n; float* pyr;
};
static const char* const kFaultNames[] = {"plan NULL", "view NULL", "data NULL", "channels 1", "channels 4", "pixel_stride 2", "row_stride below its bound",
                                          "frame_stride below its bound", "frame_stride 0", "span of 2^63 bytes", "pyr NULL", "plan of another context",
                                          "n_frames 0", "single-channel plan"};
static void refusal_table(const Args& valid, const silent_pyramid_plan* plan_other, const silent_pyramid_plan* plan_gray) {
    const int n_faults = (int)(sizeof(kFaultNames) / sizeof(kFaultNames[0]));
    for (int dev = 0; dev < 2; ++dev)
        for (int f = 0; f < n_faults; ++f) {
            Args a = valid;
            a.vp = &a.view;
            switch (f) {
                case 0: a.plan = nullptr; break;
                case 1: a.vp = nullptr; break;
                case 2: a.view.data = nullptr; break;
                case 3: a.view.channels = 1; break;
                case 4: a.view.channels = 4; break;
                case 5: a.view.pixel_stride = 2; break;
                case 6: a.view.row_stride = 56 * a.view.pixel_stride + 2; break;
                case 7: a.view.frame_stride = 39 * a.view.row_stride + 56 * a.view.pixel_stride + 2; break;
                case 8: a.view.frame_stride = 0; break;
                case 9: a.view.frame_stride = 1ll << 62; a.n = 3; break;
                case 10: a.pyr = nullptr; break;
                case 11: a.plan = plan_other; break;
                case 12: a.n = 0; break;
                case 13: a.plan = plan_gray; break;
            }
            const int rc = dev ? silent_pyramid_rgb8_view_dev(a.ctx, a.plan, a.vp, a.n, a.pyr, nullptr)
                               : silent_pyramid_rgb8_view(a.ctx, a.plan, a.vp, a.n, a.pyr);
            std::printf("%s | %s | %d | %s\n", dev ? "silent_pyramid_rgb8_view_dev" : "silent_pyramid_rgb8_view", kFaultNames[f], rc,
                        rc == SILENT_OK ? "-" : silent_last_error(a.ctx));
        }
}

// ---- --addresses
static int addresses(silent_ctx* ctx, int argc, char** argv) {
    if (argc < 5) return 2;
    const int H = std::atoi(argv[2]), W = std::atoi(argv[3]), nl = std::atoi(argv[4]), n = 2;
    if (argc != 5 + 8 * nl) return 2;
    std::vector<silent_pyr_level> levels(nl);
    for (int l = 0; l < nl; ++l) {
        int v[8];
        for (int i = 0; i < 8; ++i) v[i] = std::atoi(argv[5 + 8 * l + i]);
        levels[l] = silent_pyr_level{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    }
    silent_pyramid_plan* plan = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, levels.data(), nl, &plan), SILENT_OK);
    if (failures) return 1;
    silent::Walk3Args wa;
    if (!walk3_plan<ViewRgb>(ctx, plan, n, &wa)) {
        std::printf("%d x %d: the plan has no walk launch\n", H, W);
        return 1;
    }
    const int px = plan->walk_px, loads = silent::w3_view_row_loads(px);
    for (const Kind& k : kinds(H, W)) {
        const long long span = span_of(k, n, H, W);
        const uintptr_t base = 0x10000 + (uintptr_t)k.offset;     // (the parent 4-byte aligned, as an allocation is)
        const ViewRgb v{nullptr, k.pixel, k.row, k.frame};
        std::vector<uint8_t> touched((size_t)span, 0);
        long long n_loads = 0, outside = 0, misaligned = 0;
        for (unsigned bid = 0; bid < (unsigned)(n * wa.blocks_per_frame); ++bid) {
            const silent::W3ViewBlock b = silent::w3_view_block(wa, px, bid);
            for (int c = 0; c < b.n_chunks; ++c)
                for (int r = 0; r < silent::kW3CH; ++r)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int s = 0; s < loads; ++s) {
                            const silent::W3ViewLoad L = silent::w3_view_load(wa, v, px, bid, c, r, lane, s);
                            ++n_loads;
                            if (L.width < 1 || L.offset < 0 || L.offset + L.width > span) {
                                if (!outside++) std::printf("%s: block %u chunk %d row %d lane %d slot %d: offset %lld width %d outside [0, %lld)\n",
                                                            k.name, bid, c, r, lane, s, L.offset, L.width, span);
                                continue;
                            }
                            if (L.width > 1 && (base + (uintptr_t)L.offset) % (uintptr_t)L.width) ++misaligned;
                            for (int i = 0; i < L.width; ++i) touched[(size_t)L.offset + i] = 1;
                        }
        }
        long long missing = 0, needed = 0;
        for (int f = 0; f < n; ++f)
            for (int p = 0; p < wa.n_plans; ++p) {
                const silent::Walk3Plan& w = wa.plan[p];
                for (int y = w.src_y0; y < w.src_y0 + w.src_h; ++y)
                    for (int x = w.src_x0; x < w.src_x0 + w.src_w; ++x)
                        for (int ch = 0; ch < 3; ++ch) {
                            ++needed;
                            if (!touched[(size_t)(f * k.frame + y * k.row + x * k.pixel + ch)]) ++missing;
                        }
            }
        long long not_pixel = 0;       // bytes touched that are no channel byte of a pixel of the view (allowed inside the span; none as built)
        {
            std::vector<uint8_t> pixel((size_t)span, 0);
            for (int f = 0; f < n; ++f)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x)
                        for (int ch = 0; ch < 3; ++ch) pixel[(size_t)(f * k.frame + y * k.row + x * k.pixel + ch)] = 1;
            for (long long i = 0; i < span; ++i) not_pixel += touched[(size_t)i] && !pixel[(size_t)i];
        }
        std::printf("%d x %d | %s | plans %d px %d blocks %d | loads %lld | outside %lld | misaligned %lld | needed %lld missing %lld | not a pixel byte %lld\n",
                    H, W, k.name, wa.n_plans, px, n * wa.blocks_per_frame, n_loads, outside, misaligned, needed, missing, not_pixel);
        if (outside || misaligned || missing || !needed) ++failures;
    }
    silent_pyramid_plan_destroy(plan);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
    const int H = 40, W = 57, n = 2;
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
        if (rc == 2) std::printf("usage: --addresses H W n_levels <8 integers per level>\n");
        return rc;
    }
    const silent_pyr_level ladder[3] = {{0, 0, H, W, H, W, H, W}, {0, 0, H, W, 20, 29, 20, 29}, {0, 0, H, W, 10, 14, 10, 14}};
    const silent_pyr_level crops[3] = {{3, 5, 30, 41, 30, 41, 30, 41}, {0, 0, H, W, 20, 29, 22, 31}, {10, 16, 20, 33, 10, 17, 10, 17}};
    silent_pyramid_plan *plan = nullptr, *plan_crop = nullptr, *plan_gray = nullptr, *plan_other = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, ladder, 3, &plan), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, crops, 3, &plan_crop), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, ladder, 3, &plan_gray), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(other, H, W, 3, ladder, 3, &plan_other), SILENT_OK);
    if (failures) return 1;

    // bgra (span 18239), an odd-pitch bgr whose frames have a gap (span 14152), and a PACKED view (span 13680: the packed kernels'
    // route); none a multiple of the arena's 256-byte steps
    const Kind views[3] = {{"bgra", 0, 4, 4 * W, 4 * W * H}, {"pitch", 0, 3, 3 * W + 5, (3 * W + 5) * H + 77}, {"packed", 0, 3, 3 * W, 3 * W * H}};
    const silent_pyramid_plan* plans[2] = {plan, plan_crop};
    for (const Kind& k : views) {
        const size_t span = (size_t)span_of(k, n, H, W);
        uint8_t* data = (uint8_t*)std::malloc(span);         // EXACTLY span bytes
        for (size_t i = 0; i < span; ++i) data[i] = (uint8_t)(i * 37 + 11);
        const silent_frame_view view{data, 3, k.pixel, k.row, k.frame};
        for (const silent_pyramid_plan* p : plans) {
            const size_t px = (size_t)n * (p == plan ? 40 * 57 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
            std::vector<float> pyr(px * 3);
            if (refusals) {
                if (p == plan && &k == &views[0]) refusal_table(Args{ctx, p, view, nullptr, n, pyr.data()}, plan_other, plan_gray);
                continue;
            }
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &view, n, pyr.data()), SILENT_OK);
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, p, &view, n, pyr.data(), nullptr), SILENT_OK);
            // one frame: frame_stride is not read
            silent_frame_view one = view;
            one.frame_stride = -5;
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &one, 1, pyr.data()), SILENT_OK);
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, p, &one, 1, pyr.data(), nullptr), SILENT_OK);
            // ---- the host form stages exactly `span` bytes: the view is the first argument staged (arena offset 0, the next one starts
            // on the following multiple of 256); the arena is poisoned, the call made again
            const size_t staged_end = (span + 255) / 256 * 256;
            if (!ctx->arena.p || ctx->arena.cap < staged_end + pyr.size() * 4) {
                std::printf("the staging arena holds %zu bytes, expected at least %zu\n", (size_t)ctx->arena.cap, staged_end + pyr.size() * 4);
                ++failures;
                continue;
            }
            std::memset(ctx->arena.p, 0xEE, ctx->arena.cap);
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &view, n, pyr.data()), SILENT_OK);
            const uint8_t* arena = (const uint8_t*)ctx->arena.p;
            if (std::memcmp(arena, data, span) != 0) {
                std::printf("%s: the staged bytes differ from the view's span\n", k.name);
                ++failures;
            }
            if (span % 256 == 0) { std::printf("%s: span is a multiple of 256\n", k.name); ++failures; }
            for (size_t i = span; i < staged_end; ++i)
                if (arena[i] != 0xEE) {
                    std::printf("%s: byte %zu of the arena was written: more than span = %zu bytes were staged\n", k.name, i, span);
                    ++failures;
                    break;
                }
            // ---- status codes
            silent_frame_view bad = view;
            EXPECT(silent_pyramid_rgb8_view(ctx, nullptr, &view, n, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view(ctx, p, nullptr, n, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &view, n, nullptr), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &view, 0, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view(ctx, plan_other, &view, n, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view(ctx, plan_gray, &view, n, pyr.data()), SILENT_E_UNSUPPORTED);
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, plan_gray, &view, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
            if (!std::strstr(silent_last_error(ctx), "silent_pyramid_view)")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
            bad.channels = 1;
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &bad, n, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, p, &bad, n, pyr.data(), nullptr), SILENT_E_INVALID);
            bad = view;
            bad.row_stride = (W - 1) * k.pixel + 2;
            EXPECT(silent_pyramid_rgb8_view(ctx, p, &bad, n, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, p, &bad, n, pyr.data(), nullptr), SILENT_E_INVALID);
            // the order: the view's own refusals before the shared checks, NULL before the context, the context before n_frames, n_frames
            // before the plan's channels; a NULL ctx before everything
            EXPECT(silent_pyramid_rgb8_view(nullptr, nullptr, nullptr, 0, nullptr), SILENT_E_INVALID);
            bad = view;
            bad.channels = 1;
            EXPECT(silent_pyramid_rgb8_view(ctx, plan_gray, &bad, 0, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "channels must be 3")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad = view;
            bad.pixel_stride = 2;
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "pixel_stride")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_rgb8_view(ctx, plan_other, &view, 0, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "NULL pointer")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_rgb8_view_dev(ctx, plan_other, &view, 0, pyr.data(), nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "another context")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_rgb8_view(ctx, plan_gray, &view, 0, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "n_frames")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            // the single-channel view call still refuses a 3-channel plan, the packed colour call still takes packed bytes
            EXPECT(silent_pyramid_view(ctx, p, &view, n, pyr.data()), SILENT_E_UNSUPPORTED);
            if (&k == &views[2]) EXPECT(silent_pyramid_rgb8(ctx, p, data, n, pyr.data()), SILENT_OK);
        }
        std::free(data);
    }
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    for (silent_pyramid_plan* q : {plan, plan_crop, plan_gray, plan_other}) silent_pyramid_plan_destroy(q);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    if (!refusals) std::printf("rgb8 view host main ok\n");
    return 0;
}
