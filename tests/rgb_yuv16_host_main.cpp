// Stand-alone driver of silent_pyramid_yuv1616[_dev] and silent_yuv16_to_rgb[_dev] (planar, semi-planar and packed 16-bit YUV for
// 3-channel plans) on the library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("rgb_yuv16")).  ONE translation unit with
// silent_unity.hip, -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel launches are compiled out and device memory is host
// memory, so what runs is the argument validation, the plan tables, the host forms' staging and the walk loader's ADDRESS FUNCTION
// (w3_yuv16_load, silent_walk_rgb.h: the function the kernel forms its addresses with).
//   no argument     both forms of both entry points, for a classic and a crop plan, on I010 planes that are three heap blocks of EXACTLY
//                   their spans, on a Y210 buffer that is ONE heap block of exactly the union of its three spans, and on P010 surfaces
//                   given as a triple (a staging size above a span reads past it: AddressSanitizer reports it; one below it leaves
//                   poison in the staging arena, which this program looks at); the host forms stage exactly the MERGED spans (Y210: one
//                   interval, copied once); the status codes and the order of the checks; one "ok" line
//   --sizeof        sizeof(silent_yuv16_frames) and the offset of every field, one line
//   --refusals      "name | case | status | silent_last_error" per (entry point, single fault): tests/golden/yuv16_refusals.txt
//   --addresses LAYOUT H W n_levels <8 integers per level>
//                   every (block, chunk, row, lane, load slot) of the plan's walk launch on two frames: every offset is the EVEN offset of
//                   an element that is some pixel's Y (U, V) of that plane, and the elements touched contain the Y, U and V of every pixel
//                   of every walk plan's crop; one line, with the number of plans whose crop starts at an odd row AND an odd column
#include <cmath>
#include <cstddef>
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

// a layout: shifts, BYTE strides (all even), and the byte offsets of the three planes inside one buffer (one_buffer) or in buffers of
// their own; depth and shift of the code
struct Layout {
    int sx, sy;
    int depth, shift;
    long long yp, yr, yf, cp, cr, cf;
    long long yo, uo, vo;
    bool one_buffer;
};
static bool layout_of(const char* name, int H, int W, Layout* l) {
    const std::string s(name);
    const int sx = (s == "i410" || s == "yuv440") ? 0 : 1, sy = (s == "i010" || s == "p010" || s == "vu010" || s == "yuv440") ? 1 : 0;
    const long long ch = H >> sy, cw = W >> sx;
    *l = Layout{sx, sy, 10, 0, 2, 0, 0, 2, 0, 0, 0, 0, 0, false};
    if (s == "i010" || s == "i210" || s == "i410" || s == "yuv440") {       // three pitched planes, the code in the low bits: chroma
        l->yr = 2 * (W + 9);                                                 // pitch != luma pitch / 2, rows no multiple of 4 bytes
        l->cr = 2 * ((cw + 7) | 1);
        l->yf = l->yr * H + 334;
        l->cf = l->cr * ch + 78;
    } else if (s == "p010" || s == "vu010" || s == "p210") {                // a plane of interleaved element pairs, the code in the high bits
        l->shift = 6;
        l->yr = 2 * (W + 9);
        l->cr = 2 * (2 * cw + 23);
        l->cp = 4;
        l->yf = l->yr * H + 334;
        l->cf = l->cr * ch + 78;
        l->uo = s == "vu010" ? 2 : 0;
        l->vo = s == "vu010" ? 0 : 2;
    } else if (s == "y210") {                                               // packed 4:2:2 (Y0 U Y1 V), padded rows, one buffer
        l->shift = 6;
        l->yp = 4;
        l->cp = 8;
        l->yr = l->cr = 2 * (2 * W + 11);
        l->yf = l->cf = l->yr * H + 42;
        l->yo = 0;
        l->uo = 2;
        l->vo = 6;
        l->one_buffer = true;
    } else {
        return false;
    }
    return true;
}
static long long y_span(const Layout& l, int n, int H, int W) { return (n - 1) * l.yf + (long long)(H - 1) * l.yr + (long long)(W - 1) * l.yp + 2; }
static long long c_span(const Layout& l, int n, int H, int W) {
    return (n - 1) * l.cf + (long long)((H >> l.sy) - 1) * l.cr + (long long)((W >> l.sx) - 1) * l.cp + 2;
}
static silent_yuv16_frames frames_of(const uint8_t* y, const uint8_t* u, const uint8_t* v, const Layout& l) {
    silent_yuv16_frames f;
    f.y = reinterpret_cast<const uint16_t*>(y);
    f.u = reinterpret_cast<const uint16_t*>(u);
    f.v = reinterpret_cast<const uint16_t*>(v);
    f.y_pixel_stride = l.yp;
    f.y_row_stride = l.yr;
    f.y_frame_stride = l.yf;
    f.c_pixel_stride = l.cp;
    f.c_row_stride = l.cr;
    f.c_frame_stride = l.cf;
    f.chroma_shift_x = l.sx;
    f.chroma_shift_y = l.sy;
    const float m[9] = {1.164f, 2.112f, 0.0f, 1.164f, -0.213f, -0.533f, 1.164f, 0.0f, 1.793f};
    for (int i = 0; i < 9; ++i) f.m[i] = m[i] * 0.25f;
    f.oy = 64.0f;
    f.oc = 512.0f;
    f.shift = l.shift;
    f.depth = l.depth;
    return f;
}

struct Args {
    silent_ctx* ctx; const silent_pyramid_plan* plan; silent_yuv16_frames f; const silent_yuv16_frames* fp; int n, H, W; float* out;
};
static const char* const kFaultNames[] = {"plan NULL", "struct NULL", "y NULL", "u NULL", "v NULL", "chroma_shift_x 2", "chroma_shift_y -1",
                                          "odd H", "odd W", "y_pixel_stride 1", "c_pixel_stride -2", "y_row_stride below its row extent",
                                          "c_row_stride below its row extent", "y_frame_stride below its bound", "c_frame_stride below its bound",
                                          "y_frame_stride 0", "span of 2^63 bytes", "m not finite", "oy not finite", "oc not finite",
                                          "odd y address", "odd v address", "odd y_pixel_stride", "odd c_row_stride", "odd c_frame_stride",
                                          "depth 7", "depth 17", "shift -1", "shift + depth 17", "out NULL",
                                          "plan of another context", "n_frames 0", "single-channel plan"};
static void refusal_table(const Args& valid, const silent_pyramid_plan* plan_odd_h, const silent_pyramid_plan* plan_odd_w,
                          const silent_pyramid_plan* plan_other, const silent_pyramid_plan* plan_gray) {
    const int n_faults = (int)(sizeof(kFaultNames) / sizeof(kFaultNames[0]));
    const char* const names[4] = {"silent_pyramid_yuv16", "silent_pyramid_yuv16_dev", "silent_yuv16_to_rgb", "silent_yuv16_to_rgb_dev"};
    for (int e = 0; e < 4; ++e)
        for (int k = 0; k < n_faults; ++k) {
            const bool pyramid = e < 2;
            if (!pyramid && (k == 0 || k == 30 || k == 32)) continue;      // (no plan argument)
            Args a = valid;
            a.fp = &a.f;
            const long long cw = valid.W >> a.f.chroma_shift_x, chh = valid.H >> a.f.chroma_shift_y;
            switch (k) {
                case 0: a.plan = nullptr; break;
                case 1: a.fp = nullptr; break;
                case 2: a.f.y = nullptr; break;
                case 3: a.f.u = nullptr; break;
                case 4: a.f.v = nullptr; break;
                case 5: a.f.chroma_shift_x = 2; break;
                case 6: a.f.chroma_shift_y = -1; break;
                case 7: a.plan = plan_odd_h; a.H = valid.H - 1; break;
                case 8: a.plan = plan_odd_w; a.W = valid.W - 1; break;
                case 9: a.f.y_pixel_stride = 1; break;
                case 10: a.f.c_pixel_stride = -2; break;
                case 11: a.f.y_row_stride = (valid.W - 1) * a.f.y_pixel_stride; break;
                case 12: a.f.c_row_stride = (cw - 1) * a.f.c_pixel_stride; break;
                case 13: a.f.y_frame_stride = (valid.H - 1) * a.f.y_row_stride + (valid.W - 1) * a.f.y_pixel_stride; break;
                case 14: a.f.c_frame_stride = (chh - 1) * a.f.c_row_stride + (cw - 1) * a.f.c_pixel_stride; break;
                case 15: a.f.y_frame_stride = 0; break;
                case 16: a.f.c_frame_stride = 1ll << 62; a.n = 3; break;
                case 17: a.f.m[4] = std::numeric_limits<float>::quiet_NaN(); break;
                case 18: a.f.oy = std::numeric_limits<float>::infinity(); break;
                case 19: a.f.oc = -std::numeric_limits<float>::infinity(); break;
                case 20: a.f.y = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.f.y) + 1); break;
                case 21: a.f.v = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.f.v) + 1); break;
                case 22: a.f.y_pixel_stride = 3; a.f.y_row_stride += 2 * valid.W; a.f.y_frame_stride += 2 * valid.W * valid.H; break;
                case 23: a.f.c_row_stride += 1; a.f.c_frame_stride += 2 * chh; break;
                case 24: a.f.c_frame_stride += 1; break;
                case 25: a.f.depth = 7; a.f.shift = 0; break;
                case 26: a.f.depth = 17; a.f.shift = 0; break;
                case 27: a.f.shift = -1; break;
                case 28: a.f.depth = 12; a.f.shift = 5; break;
                case 29: a.out = nullptr; break;
                case 30: a.plan = plan_other; break;
                case 31: a.n = 0; break;
                case 32: a.plan = plan_gray; break;
            }
            int rc;
            if (e == 0) rc = silent_pyramid_yuv16(a.ctx, a.plan, a.fp, a.n, a.out);
            else if (e == 1) rc = silent_pyramid_yuv16_dev(a.ctx, a.plan, a.fp, a.n, a.out, nullptr);
            else if (e == 2) rc = silent_yuv16_to_rgb(a.ctx, a.fp, a.n, a.H, a.W, a.out);
            else rc = silent_yuv16_to_rgb_dev(a.ctx, a.fp, a.n, a.H, a.W, a.out, nullptr);
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
    if (!walk3_plan<Yuv16>(ctx, plan, n, &wa)) {
        std::printf("%d x %d: the plan has no walk launch\n", H, W);
        return 1;
    }
    const int px = plan->walk_px, loads = silent::w3_nv12_row_loads(px);
    const long long ys = y_span(lay, n, H, W), cs = c_span(lay, n, H, W);
    // the kernels' argument with the planes at address 0 (offsets only: the struct is built by hand, with_yuv16 is not what is
    // enumerated here)
    Yuv16 v;
    std::memset(&v, 0, sizeof(v));
    v.y_pixel_stride = lay.yp;
    v.y_row_stride = lay.yr;
    v.y_frame_stride = lay.yf;
    v.c_pixel_stride = lay.cp;
    v.c_row_stride = lay.cr;
    v.c_frame_stride = lay.cf;
    v.sx = lay.sx;
    v.sy = lay.sy;
    std::vector<uint8_t> ty((size_t)ys, 0), tu((size_t)cs, 0), tv((size_t)cs, 0);
    long long n_loads = 0, outside = 0, odd = 0;
    for (unsigned bid = 0; bid < (unsigned)(n * wa.blocks_per_frame); ++bid) {
        const silent::W3ViewBlock b = silent::w3_view_block(wa, px, bid);
        for (int c = 0; c < b.n_chunks; ++c)
            for (int r = 0; r < silent::kW3CH; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    for (int k = 0; k < loads; ++k) {
                        const silent::W3YuvLoad L = silent::w3_yuv16_load(wa, v, px, bid, c, r, lane, k);
                        ++n_loads;
                        odd += (L.y_offset & 1) + (L.u_offset & 1) + (L.v_offset & 1);
                        if (L.y_offset < 0 || L.y_offset + 2 > ys || L.u_offset < 0 || L.u_offset + 2 > cs || L.v_offset < 0 || L.v_offset + 2 > cs) {
                            if (!outside++) std::printf("block %u chunk %d row %d lane %d slot %d: y offset %lld of %lld, u offset %lld, v offset %lld of %lld\n",
                                                        bid, c, r, lane, k, L.y_offset, ys, L.u_offset, L.v_offset, cs);
                            continue;
                        }
                        ty[(size_t)L.y_offset] = 1;
                        tu[(size_t)L.u_offset] = 1;
                        tv[(size_t)L.v_offset] = 1;
                    }
    }
    long long needed = 0, missing_y = 0, missing_u = 0, missing_v = 0;
    int odd_origin = 0;
    for (int p = 0; p < wa.n_plans; ++p) odd_origin += (wa.plan[p].src_x0 & 1) && (wa.plan[p].src_y0 & 1);
    for (int f = 0; f < n; ++f)
        for (int p = 0; p < wa.n_plans; ++p) {
            const silent::Walk3Plan& w = wa.plan[p];
            for (int y = w.src_y0; y < w.src_y0 + w.src_h; ++y)
                for (int x = w.src_x0; x < w.src_x0 + w.src_w; ++x) {
                    ++needed;
                    if (!ty[(size_t)(f * lay.yf + y * lay.yr + x * lay.yp)]) ++missing_y;
                    const size_t c = (size_t)(f * lay.cf + (y >> lay.sy) * lay.cr + (x >> lay.sx) * lay.cp);
                    if (!tu[c]) ++missing_u;
                    if (!tv[c]) ++missing_v;
                }
        }
    // elements touched (marked at their first byte) that are no pixel's Y / U / V (none: every address is formed from a pixel of the
    // frame) -- stricter than "inside the span": in a packed buffer the elements between the pixels of a plane belong to the other
    // planes or to nobody
    long long not_pixel = 0;
    {
        std::vector<uint8_t> py((size_t)ys, 0), pc((size_t)cs, 0);
        for (int f = 0; f < n; ++f)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    py[(size_t)(f * lay.yf + y * lay.yr + x * lay.yp)] = 1;
                    pc[(size_t)(f * lay.cf + (y >> lay.sy) * lay.cr + (x >> lay.sx) * lay.cp)] = 1;
                }
        for (long long i = 0; i < ys; ++i) not_pixel += ty[(size_t)i] && !py[(size_t)i];
        for (long long i = 0; i < cs; ++i) not_pixel += (tu[(size_t)i] && !pc[(size_t)i]) + (tv[(size_t)i] && !pc[(size_t)i]);
    }
    std::printf("%s %d x %d | plans %d px %d blocks %d | loads %lld | outside %lld | needed %lld missing y %lld u %lld v %lld | not a pixel element %lld | odd origins %d | odd offsets %lld\n",
                argv[2], H, W, wa.n_plans, px, n * wa.blocks_per_frame, n_loads, outside, needed, missing_y, missing_u, missing_v, not_pixel, odd_origin, odd);
    if (odd || outside || missing_y || missing_u || missing_v || not_pixel || !needed) ++failures;
    silent_pyramid_plan_destroy(plan);
    return failures ? 1 : 0;
}

// what yuv_stage must make of a struct: the merged intervals, here restated with a byte map over the address range of the planes
static void check_staging(silent_ctx* ctx, const char* what, const silent_yuv16_frames& fr, size_t ys, size_t cs, int expect_intervals) {
    const YuvStage st = yuv_stage(&fr, ys, cs);
    if (st.n != expect_intervals) { std::printf("%s: %d merged intervals, expected %d\n", what, st.n, expect_intervals); ++failures; }
    const uint8_t* const p[3] = {reinterpret_cast<const uint8_t*>(fr.y), reinterpret_cast<const uint8_t*>(fr.u), reinterpret_cast<const uint8_t*>(fr.v)};
    const size_t len[3] = {ys, cs, cs};
    size_t total = 0;
    for (int i = 0; i < st.n; ++i) {
        total += st.bytes[i];
        if (i && st.start[i] <= st.start[i - 1] + st.bytes[i - 1]) { std::printf("%s: intervals %d and %d overlap, touch or are unsorted\n", what, i - 1, i); ++failures; }
    }
    for (int k = 0; k < 3; ++k) {
        const int i = st.of[k];
        if (st.start[i] + st.delta[k] != p[k] || st.delta[k] + len[k] > st.bytes[i]) { std::printf("%s: plane %d is not inside its interval\n", what, k); ++failures; }
    }
    // every byte of an interval belongs to a span: the union, not a hull
    for (int i = 0; i < st.n; ++i)
        for (size_t b = 0; b < st.bytes[i]; b += (st.bytes[i] > 4096 ? 97 : 1)) {
            const uint8_t* a = st.start[i] + b;
            bool in = false;
            for (int k = 0; k < 3; ++k) in = in || (a >= p[k] && a < p[k] + len[k]);
            if (!in) { std::printf("%s: byte %zu of interval %d belongs to no span\n", what, b, i); ++failures; break; }
        }
    (void)ctx;
    (void)total;
}

// the host form stages exactly the merged intervals: in address order from arena offset 0, each on the following multiple of 256, the
// output behind them; the arena is poisoned, the call made, the bytes compared and the poison between the intervals looked at
template <class Call>
static void check_arena(silent_ctx* ctx, const char* what, const silent_yuv16_frames& fr, size_t ys, size_t cs, size_t out_bytes, Call&& call) {
    const YuvStage st = yuv_stage(&fr, ys, cs);
    size_t at[4] = {0, 0, 0, 0};
    for (int i = 0; i < st.n; ++i) at[i + 1] = at[i] + (st.bytes[i] + 255) / 256 * 256;
    if (!ctx->arena.p || ctx->arena.cap < at[st.n] + out_bytes) {
        std::printf("%s: the staging arena holds %zu bytes, expected at least %zu\n", what, (size_t)ctx->arena.cap, at[st.n] + out_bytes);
        ++failures;
        return;
    }
    std::memset(ctx->arena.p, 0xEE, ctx->arena.cap);
    EXPECT(call(), SILENT_OK);
    const uint8_t* arena = (const uint8_t*)ctx->arena.p;
    for (int i = 0; i < st.n; ++i) {
        if (std::memcmp(arena + at[i], st.start[i], st.bytes[i]) != 0) { std::printf("%s: the staged bytes of interval %d differ\n", what, i); ++failures; }
        if (st.bytes[i] % 256 == 0) { std::printf("%s: an interval is a multiple of 256\n", what); ++failures; }
        for (size_t b = at[i] + st.bytes[i]; b < at[i + 1]; ++b)
            if (arena[b] != 0xEE) { std::printf("%s: byte %zu of the arena was written: more than %zu bytes of interval %d were staged\n", what, b, st.bytes[i], i); ++failures; break; }
    }
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
    const int H = 40, W = 58, n = 2;
    if (argc > 1 && !std::strcmp(argv[1], "--sizeof")) {
        typedef silent_yuv16_frames S;
        std::printf("sizeof %zu | y %zu u %zu v %zu y_pixel_stride %zu y_row_stride %zu y_frame_stride %zu c_pixel_stride %zu c_row_stride %zu "
                    "c_frame_stride %zu chroma_shift_x %zu chroma_shift_y %zu m %zu oy %zu oc %zu shift %zu depth %zu\n",
                    sizeof(S), offsetof(S, y), offsetof(S, u), offsetof(S, v), offsetof(S, y_pixel_stride), offsetof(S, y_row_stride),
                    offsetof(S, y_frame_stride), offsetof(S, c_pixel_stride), offsetof(S, c_row_stride), offsetof(S, c_frame_stride),
                    offsetof(S, chroma_shift_x), offsetof(S, chroma_shift_y), offsetof(S, m), offsetof(S, oy), offsetof(S, oc),
                    offsetof(S, shift), offsetof(S, depth));
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
    const silent_pyr_level ladder_odd_h[1] = {{0, 0, H - 1, W, H - 1, W, H - 1, W}}, ladder_odd_w[1] = {{0, 0, H, W - 1, H, W - 1, H, W - 1}};
    silent_pyramid_plan *plan = nullptr, *plan_crop = nullptr, *plan_gray = nullptr, *plan_other = nullptr, *plan_odd_h = nullptr, *plan_odd_w = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, ladder, 3, &plan), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, crops, 3, &plan_crop), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, ladder, 3, &plan_gray), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(other, H, W, 3, ladder, 3, &plan_other), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H - 1, W, 3, ladder_odd_h, 1, &plan_odd_h), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W - 1, 3, ladder_odd_w, 1, &plan_odd_w), SILENT_OK);
    if (failures) return 1;

    // the three test batches: I010 in three heap blocks of EXACTLY the spans; Y210 in ONE heap block of exactly the union of its spans
    // (which ends with the V element of the last pixel); P010 surfaces as a triple (v == u + 1 element: the P010 kernels' dispatch) in
    // two blocks, the chroma block exactly the union of the U span and the V span
    const char* const kinds[3] = {"i010", "y210", "p010"};
    std::vector<float> rgb((size_t)n * H * W * 3);
    for (int kind = 0; kind < 3; ++kind) {
        Layout lay;
        layout_of(kinds[kind], H, W, &lay);
        const size_t ys = (size_t)y_span(lay, n, H, W), cs = (size_t)c_span(lay, n, H, W);
        uint8_t* blocks[3] = {nullptr, nullptr, nullptr};
        silent_yuv16_frames fr;
        int expect_intervals;
        if (kind == 0) {
            blocks[0] = (uint8_t*)std::malloc(ys);
            blocks[1] = (uint8_t*)std::malloc(cs);
            blocks[2] = (uint8_t*)std::malloc(cs);
            for (size_t i = 0; i < ys; ++i) blocks[0][i] = (uint8_t)(i * 37 + 11);
            for (size_t i = 0; i < cs; ++i) blocks[1][i] = (uint8_t)(i * 101 + 7), blocks[2][i] = (uint8_t)(i * 53 + 3);
            fr = frames_of(blocks[0], blocks[1], blocks[2], lay);
            expect_intervals = 3;
        } else if (kind == 1) {
            const size_t all = (size_t)lay.vo + cs;               // = (n - 1) frame + (H - 1) row + 4 W
            if (all != (size_t)((n - 1) * lay.yf + (H - 1) * lay.yr + 4 * W) || (size_t)lay.yo + ys > all || (size_t)lay.uo + cs > all) { std::printf("y210 union\n"); ++failures; }
            blocks[0] = (uint8_t*)std::malloc(all);
            for (size_t i = 0; i < all; ++i) blocks[0][i] = (uint8_t)(i * 37 + 11);
            fr = frames_of(blocks[0] + lay.yo, blocks[0] + lay.uo, blocks[0] + lay.vo, lay);
            expect_intervals = 1;
        } else {
            blocks[0] = (uint8_t*)std::malloc(ys);
            blocks[1] = (uint8_t*)std::malloc(cs + 2);
            for (size_t i = 0; i < ys; ++i) blocks[0][i] = (uint8_t)(i * 37 + 11);
            for (size_t i = 0; i < cs + 2; ++i) blocks[1][i] = (uint8_t)(i * 101 + 7);
            fr = frames_of(blocks[0], blocks[1] + lay.uo, blocks[1] + lay.vo, lay);
            expect_intervals = 2;
        }
        check_staging(ctx, kinds[kind], fr, ys, cs, expect_intervals);
        const silent_pyramid_plan* plans[2] = {plan, plan_crop};
        for (const silent_pyramid_plan* p : plans) {
            const size_t px = (size_t)n * (p == plan ? 40 * 58 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
            std::vector<float> pyr(px * 3);
            if (refusals) {
                if (p == plan && kind == 0) refusal_table(Args{ctx, p, fr, nullptr, n, H, W, pyr.data()}, plan_odd_h, plan_odd_w, plan_other, plan_gray);
                continue;
            }
            EXPECT(silent_pyramid_yuv16(ctx, p, &fr, n, pyr.data()), SILENT_OK);
            EXPECT(silent_pyramid_yuv16_dev(ctx, p, &fr, n, pyr.data(), nullptr), SILENT_OK);
            EXPECT(silent_yuv16_to_rgb(ctx, &fr, n, H, W, rgb.data()), SILENT_OK);
            EXPECT(silent_yuv16_to_rgb_dev(ctx, &fr, n, H, W, rgb.data(), nullptr), SILENT_OK);
            check_arena(ctx, kinds[kind], fr, ys, cs, pyr.size() * 4, [&] { return silent_pyramid_yuv16(ctx, p, &fr, n, pyr.data()); });
            check_arena(ctx, kinds[kind], fr, ys, cs, rgb.size() * 4, [&] { return silent_yuv16_to_rgb(ctx, &fr, n, H, W, rgb.data()); });
            if (kind != 0) continue;
            // one frame: the frame strides are not read (three blocks of exactly the one-frame spans)
            {
                const size_t ys1 = (size_t)y_span(lay, 1, H, W), cs1 = (size_t)c_span(lay, 1, H, W);
                uint8_t *a = (uint8_t*)std::malloc(ys1), *b = (uint8_t*)std::malloc(cs1), *c = (uint8_t*)std::malloc(cs1);
                std::memset(a, 90, ys1);
                std::memset(b, 100, cs1);
                std::memset(c, 200, cs1);
                silent_yuv16_frames one = frames_of(a, b, c, lay);
                one.y_frame_stride = -5;
                one.c_frame_stride = 0;
                EXPECT(silent_pyramid_yuv16(ctx, p, &one, 1, pyr.data()), SILENT_OK);
                EXPECT(silent_pyramid_yuv16_dev(ctx, p, &one, 1, pyr.data(), nullptr), SILENT_OK);
                EXPECT(silent_yuv16_to_rgb(ctx, &one, 1, H, W, rgb.data()), SILENT_OK);
                std::free(a);
                std::free(b);
                std::free(c);
            }
            // ---- status codes and the order of the checks: a NULL ctx before everything; the struct's own refusals in the header's
            // order and before the shared checks; NULL before the context, the context before n_frames, n_frames before the channels
            silent_yuv16_frames bad = fr;
            EXPECT(silent_pyramid_yuv16(nullptr, nullptr, nullptr, 0, nullptr), SILENT_E_INVALID);
            EXPECT(silent_yuv16_to_rgb_dev(nullptr, nullptr, 0, 0, 0, nullptr, nullptr), SILENT_E_INVALID);
            EXPECT(silent_pyramid_yuv16(ctx, plan_gray, &fr, n, pyr.data()), SILENT_E_UNSUPPORTED);
            EXPECT(silent_pyramid_yuv16_dev(ctx, plan_gray, &fr, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
            if (!std::strstr(silent_last_error(ctx), "silent_pyramid_view16)")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
            bad.c_row_stride = 4;
            EXPECT(silent_pyramid_yuv16_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "c_row_stride")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.y_pixel_stride = 1;                                   // a pixel stride before a row stride
            EXPECT(silent_pyramid_yuv16_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "pixel stride")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.chroma_shift_x = 3;                                   // a shift before a pixel stride
            EXPECT(silent_pyramid_yuv16_dev(ctx, plan_other, &bad, 0, nullptr, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "chroma shift")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad = fr;
            bad.depth = 3;                                            // the coefficients before the alignment, the alignment before the depth
            bad.y_row_stride += 1;
            EXPECT(silent_pyramid_yuv16(ctx, p, &bad, 1, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "a stride is odd")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.u = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(bad.u) + 1);
            EXPECT(silent_pyramid_yuv16(ctx, p, &bad, 1, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "2-byte aligned")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad.oc = std::numeric_limits<float>::quiet_NaN();
            EXPECT(silent_pyramid_yuv16(ctx, p, &bad, 1, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "must be finite")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            bad = fr;
            bad.m[0] = std::numeric_limits<float>::infinity();        // the span before the coefficients
            bad.y_frame_stride = 1ll << 62;
            EXPECT(silent_pyramid_yuv16(ctx, p, &bad, 3, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "2^63")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_yuv16(ctx, plan_other, &fr, 0, nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "NULL pointer")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_yuv16_dev(ctx, plan_other, &fr, 0, pyr.data(), nullptr), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "another context")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_pyramid_yuv16(ctx, plan_gray, &fr, 0, pyr.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "n_frames")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
            EXPECT(silent_yuv16_to_rgb(ctx, &fr, n, H + 1, W, rgb.data()), SILENT_E_INVALID);
            if (!std::strstr(silent_last_error(ctx), "even extent")) { std::printf("text: %s\n", silent_last_error(ctx)); ++failures; }
            // odd extents where the format allows them: 4:4:4 takes odd H and W (planes of exactly the spans)
            {
                Layout l4;
                layout_of("i410", H - 1, W - 1, &l4);
                const size_t a4 = (size_t)y_span(l4, n, H - 1, W - 1), c4 = (size_t)c_span(l4, n, H - 1, W - 1);
                uint8_t *a = (uint8_t*)std::malloc(a4), *b = (uint8_t*)std::malloc(c4), *c = (uint8_t*)std::malloc(c4);
                std::memset(a, 90, a4);
                std::memset(b, 100, c4);
                std::memset(c, 200, c4);
                const silent_yuv16_frames f4 = frames_of(a, b, c, l4);
                EXPECT(silent_yuv16_to_rgb(ctx, &f4, n, H - 1, W - 1, rgb.data()), SILENT_OK);
                std::free(a);
                std::free(b);
                std::free(c);
            }
            // depths the Python names do not reach: 9 and 8 in the low bits, 14 in bits 1 .. 14
            for (int d = 0; d < 3; ++d) {
                silent_yuv16_frames odd_depth = fr;
                odd_depth.depth = d == 0 ? 9 : (d == 1 ? 8 : 14);
                odd_depth.shift = d == 2 ? 1 : 0;
                EXPECT(silent_yuv16_to_rgb(ctx, &odd_depth, n, H, W, rgb.data()), SILENT_OK);
                EXPECT(silent_pyramid_yuv16_dev(ctx, p, &odd_depth, n, pyr.data(), nullptr), SILENT_OK);
            }
            // the float32 call still takes what it took
            EXPECT(silent_pyramid(ctx, p, rgb.data(), n, pyr.data()), SILENT_OK);
        }
        for (uint8_t* b : blocks) std::free(b);
    }
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
    if (!refusals) std::printf("rgb yuv16 host main ok\n");
    return 0;
}
