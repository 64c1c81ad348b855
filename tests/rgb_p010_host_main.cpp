// Stand-alone driver of silent_pyramid_p010[_dev] and silent_p010_to_rgb[_dev] (P010 / P012 / P016 decoder surfaces for 3-channel
// plans) on the library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("rgb_p010")).  ONE translation unit with
// silent_unity.hip, -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel launches are compiled out and device memory is host
// memory, so what runs is the argument validation, the plan tables, the host forms' staging and the walk loader's ADDRESS FUNCTION
// (w3_p010_load, silent_walk_rgb.h: the function the kernel forms its addresses with).
//   no argument     both forms of both entry points on planes that are heap blocks of EXACTLY their spans (a staging size above a span
//                   reads past it: AddressSanitizer reports it; one below it leaves poison in the staging arena, which this program
//                   looks at), for a classic and a crop plan; the status codes and the order of the checks; one "ok" line
//   --refusals      "name | case | status | silent_last_error" per (entry point, single fault): tests/golden/p010_refusals.txt
//   --addresses H W n_levels <8 integers per level>
//                   every (block, chunk, row, lane, load slot) of the plan's walk launch on two frames: every access (2 luma bytes, 4
//                   chroma bytes) inside its plane's span and 2-byte aligned, the bytes touched contain the luma element of every
//                   pixel of every walk plan's crop and the pair of elements under it, and no byte is touched that is not a pixel's;
//                   one line, with the number of plans whose crop starts at an odd row AND an odd column
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

// BYTE pitches and frame strides of the test surfaces (all even): the chroma pitch differs from the luma pitch, no frame stride is
// rows x pitch
struct Strides {
    long long yr, yf, ur, uf;
};
static Strides strides_of(int H, int W) {
    const long long yr = 2 * W + 18, ur = 2 * W + 44;
    return Strides{yr, yr * H + 334, ur, ur * (H / 2) + 78};
}
static long long y_span(const Strides& s, int n, int H, int W) { return (n - 1) * s.yf + (long long)(H - 1) * s.yr + 2 * W; }
static long long uv_span(const Strides& s, int n, int H, int W) { return (n - 1) * s.uf + (long long)(H / 2 - 1) * s.ur + 2 * W; }
static silent_p010_frames frames_of(const uint16_t* y, const uint16_t* uv, const Strides& s) {
    silent_p010_frames f;
    f.y = y;
    f.uv = uv;
    f.y_row_stride = s.yr;
    f.y_frame_stride = s.yf;
    f.uv_row_stride = s.ur;
    f.uv_frame_stride = s.uf;
    const float m[9] = {0.291f, 0.528f, 0.0f, 0.291f, -0.05325f, -0.13325f, 0.291f, 0.0f, 0.44825f};
    for (int i = 0; i < 9; ++i) f.m[i] = m[i];
    f.oy = 64.0f;
    f.oc = 512.0f;
    f.shift = 6;
    return f;
}

struct Args {
    silent_ctx* ctx; const silent_pyramid_plan* plan; silent_p010_frames f; const silent_p010_frames* fp; int n, H, W; float* out;
};
static const char* const kFaultNames[] = {"plan NULL", "struct NULL", "y NULL", "uv NULL", "odd H", "odd W", "y_row_stride below 2 W",
                                          "uv_row_stride below 2 W", "y_frame_stride below its bound", "uv_frame_stride below its bound",
                                          "y_frame_stride 0", "span of 2^63 bytes", "m not finite", "oy not finite", "oc not finite",
                                          "y address odd", "uv address odd", "y_row_stride odd", "uv_row_stride odd", "y_frame_stride odd",
                                          "uv_frame_stride odd", "shift -1", "shift 7", "out NULL", "plan of another context", "n_frames 0",
                                          "single-channel plan"};
static void refusal_table(const Args& valid, const silent_pyramid_plan* plan_odd_h, const silent_pyramid_plan* plan_odd_w,
                          const silent_pyramid_plan* plan_other, const silent_pyramid_plan* plan_gray) {
    const int n_faults = (int)(sizeof(kFaultNames) / sizeof(kFaultNames[0]));
    const char* const names[4] = {"silent_pyramid_p010", "silent_pyramid_p010_dev", "silent_p010_to_rgb", "silent_p010_to_rgb_dev"};
    for (int e = 0; e < 4; ++e)
        for (int k = 0; k < n_faults; ++k) {
            const bool pyramid = e < 2;
            if (!pyramid && (k == 0 || k == 24 || k == 26)) continue;      // (no plan argument)
            Args a = valid;
            a.fp = &a.f;
            switch (k) {
                case 0: a.plan = nullptr; break;
                case 1: a.fp = nullptr; break;
                case 2: a.f.y = nullptr; break;
                case 3: a.f.uv = nullptr; break;
                case 4: a.plan = plan_odd_h; a.H = valid.H - 1; break;
                case 5: a.plan = plan_odd_w; a.W = valid.W - 1; break;
                case 6: a.f.y_row_stride = 2 * valid.W - 2; break;
                case 7: a.f.uv_row_stride = 2 * valid.W - 2; break;
                case 8: a.f.y_frame_stride = (valid.H - 1) * a.f.y_row_stride + 2 * valid.W - 2; break;
                case 9: a.f.uv_frame_stride = (valid.H / 2 - 1) * a.f.uv_row_stride + 2 * valid.W - 2; break;
                case 10: a.f.y_frame_stride = 0; break;
                case 11: a.f.uv_frame_stride = 1ll << 62; a.n = 3; break;
                case 12: a.f.m[4] = std::numeric_limits<float>::quiet_NaN(); break;
                case 13: a.f.oy = std::numeric_limits<float>::infinity(); break;
                case 14: a.f.oc = -std::numeric_limits<float>::infinity(); break;
                case 15: a.f.y = (const uint16_t*)((const char*)a.f.y + 1); break;      // (refused before anything is read)
                case 16: a.f.uv = (const uint16_t*)((const char*)a.f.uv + 1); break;
                case 17: a.f.y_row_stride += 1; break;
                case 18: a.f.uv_row_stride += 1; break;
                case 19: a.f.y_frame_stride += 1; break;
                case 20: a.f.uv_frame_stride += 1; break;
                case 21: a.f.shift = -1; break;
                case 22: a.f.shift = 7; break;
                case 23: a.out = nullptr; break;
                case 24: a.plan = plan_other; break;
                case 25: a.n = 0; break;
                case 26: a.plan = plan_gray; break;
            }
            int rc;
            if (e == 0) rc = silent_pyramid_p010(a.ctx, a.plan, a.fp, a.n, a.out);
            else if (e == 1) rc = silent_pyramid_p010_dev(a.ctx, a.plan, a.fp, a.n, a.out, nullptr);
            else if (e == 2) rc = silent_p010_to_rgb(a.ctx, a.fp, a.n, a.H, a.W, a.out);
            else rc = silent_p010_to_rgb_dev(a.ctx, a.fp, a.n, a.H, a.W, a.out, nullptr);
            std::printf("%s | %s | %d | %s\n", names[e], kFaultNames[k], rc, rc == SILENT_OK ? "-" : silent_last_error(a.ctx));
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
    if (!walk3_plan<P010>(ctx, plan, n, &wa)) {
        std::printf("%d x %d: the plan has no walk launch\n", H, W);
        return 1;
    }
    const int px = plan->walk_px, loads = silent::w3_nv12_row_loads(px);
    const Strides s = strides_of(H, W);
    const long long ys = y_span(s, n, H, W), us = uv_span(s, n, H, W);
    const silent_p010_frames host = frames_of(nullptr, nullptr, s);
    const P010 v = p010_frames(&host, nullptr, nullptr, n);
    std::vector<uint8_t> ty((size_t)ys, 0), tu((size_t)us, 0);
    long long n_loads = 0, outside = 0, unaligned = 0;
    for (unsigned bid = 0; bid < (unsigned)(n * wa.blocks_per_frame); ++bid) {
        const silent::W3ViewBlock b = silent::w3_view_block(wa, px, bid);
        for (int c = 0; c < b.n_chunks; ++c)
            for (int r = 0; r < silent::kW3CH; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    for (int k = 0; k < loads; ++k) {
                        const silent::W3Nv12Load L = silent::w3_p010_load(wa, v, px, bid, c, r, lane, k);
                        ++n_loads;
                        if (L.y_offset < 0 || L.y_offset + 2 > ys || L.uv_offset < 0 || L.uv_offset + 4 > us) {
                            if (!outside++) std::printf("block %u chunk %d row %d lane %d slot %d: y offset %lld of %lld, uv offset %lld of %lld\n",
                                                        bid, c, r, lane, k, L.y_offset, ys, L.uv_offset, us);
                            continue;
                        }
                        if ((L.y_offset | L.uv_offset) & 1) ++unaligned;
                        for (int i = 0; i < 2; ++i) ty[(size_t)L.y_offset + i] = 1;
                        for (int i = 0; i < 4; ++i) tu[(size_t)L.uv_offset + i] = 1;
                    }
    }
    long long needed = 0, missing_y = 0, missing_uv = 0;
    int odd_origin = 0;
    for (int p = 0; p < wa.n_plans; ++p) odd_origin += (wa.plan[p].src_x0 & 1) && (wa.plan[p].src_y0 & 1);
    for (int f = 0; f < n; ++f)
        for (int p = 0; p < wa.n_plans; ++p) {
            const silent::Walk3Plan& w = wa.plan[p];
            for (int y = w.src_y0; y < w.src_y0 + w.src_h; ++y)
                for (int x = w.src_x0; x < w.src_x0 + w.src_w; ++x) {
                    ++needed;
                    const size_t a = (size_t)(f * s.yf + y * s.yr + 2 * x);
                    if (!ty[a] || !ty[a + 1]) ++missing_y;
                    const size_t c = (size_t)(f * s.uf + (y >> 1) * s.ur + 4 * (x >> 1));
                    if (!tu[c] || !tu[c + 1] || !tu[c + 2] || !tu[c + 3]) ++missing_uv;
                }
        }
    // bytes touched that are no pixel's luma element / no pair under a pixel of the frame (none: every address is formed from a pixel)
    long long not_pixel = 0;
    {
        std::vector<uint8_t> py((size_t)ys, 0), pu((size_t)us, 0);
        for (int f = 0; f < n; ++f)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < 2 * W; ++x) {
                    py[(size_t)(f * s.yf + y * s.yr + x)] = 1;
                    pu[(size_t)(f * s.uf + (y >> 1) * s.ur + x)] = 1;
                }
        for (long long i = 0; i < ys; ++i) not_pixel += ty[(size_t)i] && !py[(size_t)i];
        for (long long i = 0; i < us; ++i) not_pixel += tu[(size_t)i] && !pu[(size_t)i];
    }
    std::printf("%d x %d | plans %d px %d blocks %d | loads %lld | outside %lld | needed %lld missing y %lld uv %lld | not a pixel byte %lld | odd origins %d | unaligned %lld\n",
                H, W, wa.n_plans, px, n * wa.blocks_per_frame, n_loads, outside, needed, missing_y, missing_uv, not_pixel, odd_origin, unaligned);
    if (outside || missing_y || missing_uv || not_pixel || unaligned || !needed) ++failures;
    silent_pyramid_plan_destroy(plan);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
    const int H = 40, W = 58, n = 2;
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
    const silent_pyr_level crops[3] = {{3, 5, 30, 41, 30, 41, 30, 41}, {0, 0, H, W, 20, 29, 22, 31}, {11, 17, 20, 33, 10, 17, 10, 17}};
    const silent_pyr_level ladder_odd_h[1] = {{0, 0, H - 1, W, H - 1, W, H - 1, W}}, ladder_odd_w[1] = {{0, 0, H, W - 1, H, W - 1, H, W - 1}};
    silent_pyramid_plan *plan = nullptr, *plan_crop = nullptr, *plan_gray = nullptr, *plan_other = nullptr, *plan_odd_h = nullptr, *plan_odd_w = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, ladder, 3, &plan), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, crops, 3, &plan_crop), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, ladder, 3, &plan_gray), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(other, H, W, 3, ladder, 3, &plan_other), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H - 1, W, 3, ladder_odd_h, 1, &plan_odd_h), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W - 1, 3, ladder_odd_w, 1, &plan_odd_w), SILENT_OK);
    if (failures) return 1;

    const Strides s = strides_of(H, W);
    const size_t ys = (size_t)y_span(s, n, H, W), us = (size_t)uv_span(s, n, H, W);
    uint16_t* y = (uint16_t*)std::malloc(ys);           // EXACTLY the two spans
    uint16_t* uv = (uint16_t*)std::malloc(us);
    for (size_t i = 0; i < ys / 2; ++i) y[i] = (uint16_t)(i * 37 * 257 + 11);
    for (size_t i = 0; i < us / 2; ++i) uv[i] = (uint16_t)(i * 101 * 263 + 7);
    const silent_p010_frames fr = frames_of(y, uv, s);
    std::vector<float> rgb((size_t)n * H * W * 3);
    const silent_pyramid_plan* plans[2] = {plan, plan_crop};
    for (const silent_pyramid_plan* p : plans) {
        const size_t px = (size_t)n * (p == plan ? 40 * 58 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
        std::vector<float> pyr(px * 3);
        if (refusals) {
            if (p == plan) refusal_table(Args{ctx, p, fr, nullptr, n, H, W, pyr.data()}, plan_odd_h, plan_odd_w, plan_other, plan_gray);
            continue;
        }
        EXPECT(silent_pyramid_p010(ctx, p, &fr, n, pyr.data()), SILENT_OK);
        EXPECT(silent_pyramid_p010_dev(ctx, p, &fr, n, pyr.data(), nullptr), SILENT_OK);
        EXPECT(silent_p010_to_rgb(ctx, &fr, n, H, W, rgb.data()), SILENT_OK);
        EXPECT(silent_p010_to_rgb_dev(ctx, &fr, n, H, W, rgb.data(), nullptr), SILENT_OK);
        // every depth's shift
        for (int shift : {0, 4, 6}) {
            silent_p010_frames d = fr;
            d.shift = shift;
            EXPECT(silent_pyramid_p010(ctx, p, &d, n, pyr.data()), SILENT_OK);
        }
        // one frame: the frame strides are not read (odd, negative, zero)
        silent_p010_frames one = fr;
        one.y_frame_stride = -5;
        one.uv_frame_stride = 0;
        EXPECT(silent_pyramid_p010(ctx, p, &one, 1, pyr.data()), SILENT_OK);
        EXPECT(silent_pyramid_p010_dev(ctx, p, &one, 1, pyr.data(), nullptr), SILENT_OK);
        EXPECT(silent_p010_to_rgb(ctx, &one, 1, H, W, rgb.data()), SILENT_OK);
        // ---- the host forms stage exactly the two spans: luma first (arena offset 0), chroma on the following multiple of 256, the
        // output behind it; the arena is poisoned, the call made again
        const size_t uv_at = (ys + 255) / 256 * 256, out_at = uv_at + (us + 255) / 256 * 256;
        for (int which = 0; which < 2; ++which) {
            const size_t out_bytes = which ? rgb.size() * 4 : pyr.size() * 4;
            if (!ctx->arena.p || ctx->arena.cap < out_at + out_bytes) {
                std::printf("the staging arena holds %zu bytes, expected at least %zu\n", (size_t)ctx->arena.cap, out_at + out_bytes);
                ++failures;
                continue;
            }
            std::memset(ctx->arena.p, 0xEE, ctx->arena.cap);
            if (which) EXPECT(silent_p010_to_rgb(ctx, &fr, n, H, W, rgb.data()), SILENT_OK);
            else EXPECT(silent_pyramid_p010(ctx, p, &fr, n, pyr.data()), SILENT_OK);
            const uint8_t* arena = (const uint8_t*)ctx->arena.p;
            if (std::memcmp(arena, y, ys) != 0 || std::memcmp(arena + uv_at, uv, us) != 0) {
                std::printf("entry %d: the staged bytes differ from the two spans\n", which);
                ++failures;
            }
            if (ys % 256 == 0 || us % 256 == 0) { std::printf("a span is a multiple of 256\n"); ++failures; }
            for (size_t i = ys; i < uv_at; ++i)
                if (arena[i] != 0xEE) { std::printf("entry %d: byte %zu of the arena was written: more than y_span = %zu bytes were staged\n", which, i, ys); ++failures; break; }
            for (size_t i = uv_at + us; i < out_at; ++i)
                if (arena[i] != 0xEE) { std::printf("entry %d: byte %zu of the arena was written: more than uv_span = %zu bytes were staged\n", which, i, us); ++failures; break; }
        }
        // ---- status codes and the order of the checks: a NULL ctx before everything; the struct's own refusals before the shared
        // checks, and among them NV12's before alignment, stride parity and shift; NULL before the context, the context before
        // n_frames, n_frames before the plan's channels
        silent_p010_frames bad = fr;
        EXPECT(silent_pyramid_p010(nullptr, nullptr, nullptr, 0, nullptr), SILENT_E_INVALID);
        EXPECT(silent_p010_to_rgb_dev(nullptr, nullptr, 0, 0, 0, nullptr, nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_p010(ctx, plan_gray, &fr, n, pyr.data()), SILENT_E_UNSUPPORTED);
        EXPECT(silent_pyramid_p010_dev(ctx, plan_gray, &fr, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
        if (!std::strstr(silent_last_error(ctx), "silent_pyramid_view16)")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
        bad.uv_row_stride = 2 * W - 4;
        EXPECT(silent_pyramid_p010_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "uv_row_stride")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        bad = fr;
        bad.shift = 9;
        bad.y_row_stride += 1;
        bad.uv = (const uint16_t*)((const char*)bad.uv + 1);
        bad.m[0] = std::numeric_limits<float>::infinity();
        EXPECT(silent_pyramid_p010(ctx, p, &bad, n, pyr.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "finite")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        bad.m[0] = 1.0f;
        EXPECT(silent_pyramid_p010(ctx, p, &bad, n, pyr.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "2-byte aligned")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        bad.uv = fr.uv;
        EXPECT(silent_pyramid_p010(ctx, p, &bad, n, pyr.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "stride is odd")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        bad.y_row_stride = fr.y_row_stride;
        EXPECT(silent_pyramid_p010(ctx, p, &bad, n, nullptr), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "shift")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        EXPECT(silent_pyramid_p010(ctx, plan_other, &fr, 0, nullptr), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "NULL pointer")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        EXPECT(silent_pyramid_p010_dev(ctx, plan_other, &fr, 0, pyr.data(), nullptr), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "another context")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        EXPECT(silent_pyramid_p010(ctx, plan_gray, &fr, 0, pyr.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "n_frames")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        EXPECT(silent_p010_to_rgb(ctx, &fr, n, H + 1, W, rgb.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "even H and W")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
        // the float32 call still takes what it took
        EXPECT(silent_pyramid(ctx, p, rgb.data(), n, pyr.data()), SILENT_OK);
    }
    std::free(y);
    std::free(uv);
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    for (silent_pyramid_plan* q : {plan, plan_crop, plan_gray, plan_other, plan_odd_h, plan_odd_w}) silent_pyramid_plan_destroy(q);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    if (!refusals) std::printf("rgb p010 host main ok\n");
    return 0;
}
