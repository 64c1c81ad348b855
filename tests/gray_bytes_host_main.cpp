// Stand-alone driver of the pyramid / gray-pass / gray-keypoints entry points on the library's HOST side, one frame type per compilation
// (pysilent_amd/csrc/build.py, build_host_driver): -DSILENT_SFX=_u8 -DSILENT_FRAME_BYTES=1, -DSILENT_SFX=_u8x3 -DSILENT_FRAME_BYTES=3, or
// -DSILENT_FRAME_BYTES=4 for the float32-frame families (silent_pyramid, silent_gray_pass[_parts | _h], silent_gray_line_end,
// silent_gray_keypoints).  ONE translation unit with silent_unity.hip, -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel
// launches are compiled out and device memory is host memory, so what runs is the argument validation, the plan tables and the host forms'
// staging.  The frames are heap blocks of EXACTLY SILENT_FRAME_BYTES * n * H * W bytes: a staging size with a larger factor reads past
// them (AddressSanitizer reports it), a smaller one is caught by the GPU tests.  No argument: every entry point + the status codes, one
// "ok" line.  --refusals: "name | case | status | silent_last_error" per (entry point, single fault), tests/golden/gray_refusals.txt.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#ifndef SILENT_HOST_ONLY
#error "host-only build: compile with -DSILENT_HOST_ONLY (no GPU is touched)"
#endif
#ifndef SILENT_FRAME_BYTES
#error "compile with -DSILENT_FRAME_BYTES=1 | 3 | 4 (and -DSILENT_SFX=_u8 | _u8x3 for 1 | 3)"
#endif
#ifndef SILENT_SFX
#define SILENT_SFX
#endif
#include "../pysilent_amd/csrc/silent_unity.hip"

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
#define STR_(x) #x
#define STR(x) STR_(x)
#define FN(base) CAT(base, SILENT_SFX)             // silent_pyramid -> silent_pyramid_u8x3
#define FN_DEV(base) CAT(FN(base), _dev)
#define NAME(base) #base STR(SILENT_SFX)
constexpr bool kFloatFrames = SILENT_FRAME_BYTES == 4;

#if SILENT_FRAME_BYTES == 4
typedef float frame_t;
// the float32-frame gray pass in the byte families' call shape: maps_f16 picks silent_gray_pass_h, `parts` silent_gray_pass_parts_dev
#define GP_PARAMS silent_ctx* ctx, const silent_pyramid_plan* plan, const float* frames, int n, const float* cs_k, const float* end_k, int k, \
                  float clip_hi, float* pyr, void* cs, void* end, int f16
#define GP_FWD ctx, plan, frames, n, cs_k, end_k, k, clip_hi, pyr
static int silent_gray_pass_any(GP_PARAMS) {
    return f16 ? silent_gray_pass_h(GP_FWD, (uint16_t*)cs, (uint16_t*)end) : silent_gray_pass(GP_FWD, (float*)cs, (float*)end);
}
static int silent_gray_pass_any_dev(GP_PARAMS, unsigned parts, silent_stream s) {
    return f16 ? silent_gray_pass_h_dev(GP_FWD, (uint16_t*)cs, (uint16_t*)end, parts, s)
               : silent_gray_pass_parts_dev(GP_FWD, (float*)cs, (float*)end, parts, s);
}
#define GRAY_PASS silent_gray_pass_any
#define GRAY_PASS_DEV silent_gray_pass_any_dev
#else
typedef uint8_t frame_t;
#define GRAY_PASS FN(silent_gray_pass)
#define GRAY_PASS_DEV FN_DEV(silent_gray_pass)
#endif
// what a 3-channel plan / a SILENT_PLAN_ACCUM_F64 plan gets: the byte frames and float16 storage refuse both as UNSUPPORTED; the
// float32 gray pass takes F64 plans and calls a 3-channel plan INVALID; silent_pyramid takes both
#define WANT_RGB(f16) (!kFloatFrames || (f16) ? SILENT_E_UNSUPPORTED : SILENT_E_INVALID)
#define WANT_F64(f16) (!kFloatFrames || (f16) ? SILENT_E_UNSUPPORTED : SILENT_OK)

static int failures = 0;

#define EXPECT(call, want)                                                                                   \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != (want)) {                                                                                 \
            std::printf("line %d: %s -> %d, expected %d (%s)\n", __LINE__, #call, rc_, (int)(want), silent_last_error(ctx)); \
            ++failures;                                                                                      \
        }                                                                                                    \
    } while (0)

// ------------------------------------------------------------------------------------------ the refusal table
// Every argument of every family, valid; a fault changes one of them.
struct Args {
    silent_ctx* ctx; silent_pyramid_plan* plan; const frame_t* frames; int n, k;
    const float *cs_k, *end_k;
    const silent_extent* levels;   // (silent_gray_line_end)
    float *pyr, *cs, *end, *peak, *spare;   // peak: NULL (selection 1 without the peak-value map); spare: a map for the faults
    unsigned parts; int pad, sel; const silent_extent* regions; int64_t *idx, *counts; size_t cap;
};
enum Fault : unsigned {
    PLAN = 1u << 0, FRAMES = 1u << 1, PYR = 1u << 2, CSK = 1u << 3, BOTH = 1u << 4, ENDBANK = 1u << 5, N0 = 1u << 6, K5 = 1u << 7,
    OTHER = 1u << 8, RGB = 1u << 9, F64 = 1u << 10, PARTS0 = 1u << 11, REGIONS = 1u << 12, COUNTS = 1u << 13, IDX = 1u << 14,
    PADNEG = 1u << 15, SEL2 = 1u << 16, PEAK0 = 1u << 17
};
static const char* const kFaultNames[18] = {"plan NULL", "frames NULL", "pyr NULL", "cs_kernel NULL", "both map outputs NULL",
                                            "end_out without end_bank", "n_frames 0", "n_orient 5", "plan of another context",
                                            "3-channel plan", "ACCUM_F64 plan", "parts 0", "regions NULL", "counts NULL",
                                            "idx NULL with a cap", "pad -1", "selection 2", "peak_value_out with selection 0"};
struct Entry {
    const char* name;
    unsigned faults;
    std::function<int(const Args&)> call;
};
#define KP_CALL(a) a.ctx, a.plan, a.frames, a.n, a.cs_k, a.end_k, a.k, 255.0f, a.pyr, a.cs, a.end, a.pad, a.sel, 0.1, a.regions, nullptr, a.peak, a.idx, a.cap, a.counts
#define GP_CALL(a) a.ctx, a.plan, a.frames, a.n, a.cs_k, a.end_k, a.k, 255.0f, a.pyr
static std::vector<Entry> entries() {
    const unsigned pyr = PLAN | FRAMES | PYR | N0 | (kFloatFrames ? 0u : RGB | F64);
    const unsigned gp = PLAN | FRAMES | PYR | CSK | BOTH | ENDBANK | N0 | K5 | RGB | (kFloatFrames ? 0u : F64);
    const unsigned le = PYR | CSK | BOTH | ENDBANK | N0 | K5;
    // (the host form of the keypoint pass takes NULL pyr / cs_out / end_out: the maps then live in the staging arena)
    const unsigned kp = PLAN | FRAMES | CSK | ENDBANK | N0 | K5 | RGB | (kFloatFrames ? 0u : F64) | REGIONS | COUNTS | IDX | PADNEG | SEL2 | PEAK0;
    std::vector<Entry> e;
    e.push_back({NAME(silent_pyramid), pyr, [](const Args& a) { return FN(silent_pyramid)(a.ctx, a.plan, a.frames, a.n, a.pyr); }});
    e.push_back({NAME(silent_pyramid) "_dev", pyr | OTHER, [](const Args& a) { return FN_DEV(silent_pyramid)(a.ctx, a.plan, a.frames, a.n, a.pyr, nullptr); }});
#if SILENT_FRAME_BYTES == 4
    e.push_back({"silent_gray_pass", gp, [](const Args& a) { return silent_gray_pass(GP_CALL(a), a.cs, a.end); }});
    e.push_back({"silent_gray_pass_dev", gp | OTHER, [](const Args& a) { return silent_gray_pass_dev(GP_CALL(a), a.cs, a.end, nullptr); }});
    e.push_back({"silent_gray_pass_parts_dev", gp | OTHER | PARTS0,
                 [](const Args& a) { return silent_gray_pass_parts_dev(GP_CALL(a), a.cs, a.end, a.parts, nullptr); }});
    e.push_back({"silent_gray_pass_h", gp | F64, [](const Args& a) { return silent_gray_pass_h(GP_CALL(a), (uint16_t*)a.cs, (uint16_t*)a.end); }});
    e.push_back({"silent_gray_pass_h_dev", gp | F64 | OTHER | PARTS0,
                 [](const Args& a) { return silent_gray_pass_h_dev(GP_CALL(a), (uint16_t*)a.cs, (uint16_t*)a.end, a.parts, nullptr); }});
    e.push_back({"silent_gray_line_end", le, [](const Args& a) {
                     return silent_gray_line_end(a.ctx, a.pyr, a.levels, 3, a.n, a.cs_k, a.end_k, a.k, 255.0f, a.cs, a.end);
                 }});
    e.push_back({"silent_gray_line_end_dev", le, [](const Args& a) {
                     return silent_gray_line_end_dev(a.ctx, a.pyr, a.levels, 3, a.n, a.cs_k, a.end_k, a.k, 255.0f, a.cs, a.end, nullptr);
                 }});
#else
    e.push_back({NAME(silent_gray_pass), gp, [](const Args& a) { return FN(silent_gray_pass)(GP_CALL(a), a.cs, a.end, 0); }});
    e.push_back({NAME(silent_gray_pass) "_dev", gp | OTHER | PARTS0,
                 [](const Args& a) { return FN_DEV(silent_gray_pass)(GP_CALL(a), a.cs, a.end, 0, a.parts, nullptr); }});
#endif
    e.push_back({NAME(silent_gray_keypoints), kp, [](const Args& a) { return FN(silent_gray_keypoints)(KP_CALL(a)); }});
    e.push_back({NAME(silent_gray_keypoints) "_dev", kp | PYR | BOTH | OTHER,
                 [](const Args& a) { return FN_DEV(silent_gray_keypoints)(KP_CALL(a), nullptr); }});
    return e;
}

// frames_rgb: the frames of the 3-channel plan (3 x the block for float32 frames, whose host forms stage H * W * C * 4 bytes a frame)
static void refusal_table(const Args& valid, silent_pyramid_plan* plan_other, silent_pyramid_plan* plan_rgb, silent_pyramid_plan* plan_f64,
                          const frame_t* frames_rgb) {
    for (const Entry& e : entries())
        for (int f = 0; f < 18; ++f) {
            if (!(e.faults & (1u << f))) continue;
            Args a = valid;
            switch (1u << f) {
                case PLAN: a.plan = nullptr; break;
                case FRAMES: a.frames = nullptr; break;
                case PYR: a.pyr = nullptr; break;
                case CSK: a.cs_k = nullptr; break;
                case BOTH: a.cs = a.end = nullptr; break;
                case ENDBANK: a.end_k = nullptr; break;
                case N0: a.n = 0; break;                   case K5: a.k = 5; break;
                case OTHER: a.plan = plan_other; break;    case F64: a.plan = plan_f64; break;
                case RGB: a.plan = plan_rgb; a.frames = frames_rgb; break;
                case PARTS0: a.parts = 0u; break;          case REGIONS: a.regions = nullptr; break;
                case COUNTS: a.counts = nullptr; break;    case IDX: a.idx = nullptr; break;
                case PADNEG: a.pad = -1; break;            case SEL2: a.sel = 2; break;
                case PEAK0: a.sel = 0; a.peak = a.spare; break;
            }
            const int rc = e.call(a);
            std::printf("%s | %s | %d | %s\n", e.name, kFaultNames[f], rc, rc == SILENT_OK ? "-" : silent_last_error(a.ctx));
        }
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
    const int H = 40, W = 57, n = 2, K = 4;
    silent_ctx* ctx = nullptr;
    silent_ctx* other = nullptr;
    if (silent_create(0, &ctx) != SILENT_OK || silent_create(0, &other) != SILENT_OK) {
        std::printf("silent_create failed\n");
        return 2;
    }
    // a classic ladder (one unit level + two general levels on the whole frame: the stream path) and a crop layout (region + fused)
    const silent_pyr_level ladder[3] = {{0, 0, H, W, H, W, H, W}, {0, 0, H, W, 20, 29, 20, 29}, {0, 0, H, W, 10, 14, 10, 14}};
    const silent_pyr_level crops[3] = {{3, 5, 30, 41, 30, 41, 30, 41}, {0, 0, H, W, 20, 29, 22, 31}, {10, 16, 20, 33, 10, 17, 10, 17}};
    silent_pyramid_plan *plan = nullptr, *plan_crop = nullptr, *plan_rgb = nullptr, *plan_f64 = nullptr, *plan_other = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, ladder, 3, &plan), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, crops, 3, &plan_crop), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, ladder, 3, &plan_rgb), SILENT_OK);
    EXPECT(silent_pyramid_plan_create_ex(ctx, H, W, 1, ladder, 3, SILENT_PLAN_ACCUM_F64, &plan_f64), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(other, H, W, 1, ladder, 3, &plan_other), SILENT_OK);
    if (failures) return 1;

    const size_t frame_bytes = (size_t)SILENT_FRAME_BYTES * n * H * W;   // exactly SILENT_FRAME_BYTES bytes per frame pixel
    frame_t* frames = (frame_t*)std::malloc(frame_bytes);
    for (size_t i = 0; i < frame_bytes / sizeof(frame_t); ++i) frames[i] = (frame_t)(uint8_t)(i * 37 + 11);
    // what a call with the 3-channel plan is given: float32 frames of 3 channels; the byte families refuse it on the same block
    frame_t* frames_rgb = kFloatFrames ? (frame_t*)std::calloc(3, frame_bytes) : frames;
    float cs_k[9], end_k[9 * 8];
    for (int i = 0; i < 9; ++i) cs_k[i] = i == 4 ? 1.0f : -0.125f;
    for (int i = 0; i < 9 * 8; ++i) end_k[i] = (float)((i % 5) - 2) * 0.25f;

    silent_pyramid_plan* plans[2] = {plan, plan_crop};
    for (silent_pyramid_plan* p : plans) {
        const size_t px = (size_t)n * (p == plan ? 40 * 57 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
        std::vector<float> pyr(px), cs(px), end(px * 8), value(px), peak(px);
        std::vector<uint16_t> cs_h(px), end_h(px * 8);
        std::vector<int64_t> idx(n * px * 4), counts(n);
        silent_extent regions[3], extents[3];
        const silent_pyr_level* lv = p == plan ? ladder : crops;
        for (int l = 0; l < 3; ++l) regions[l] = silent_extent{lv[l].out_h / 2 > 0 ? lv[l].out_h / 2 : 1, lv[l].out_w / 2 > 0 ? lv[l].out_w / 2 : 1};
        for (int l = 0; l < 3; ++l) extents[l] = silent_extent{lv[l].out_h, lv[l].out_w};
        if (refusals) {
            if (p == plan)
                refusal_table(Args{ctx, p, frames, n, K, cs_k, end_k, extents, pyr.data(), cs.data(), end.data(), nullptr, peak.data(), 3u, 2, 1, regions,
                                   idx.data(), counts.data(), px},
                              plan_other, plan_rgb, plan_f64, frames_rgb);
            continue;
        }
        // ---- every entry point of the family, host and _dev form (device memory is host memory here)
        EXPECT(FN(silent_pyramid)(ctx, p, frames, n, pyr.data()), SILENT_OK);
        EXPECT(FN_DEV(silent_pyramid)(ctx, p, frames, n, pyr.data(), nullptr), SILENT_OK);
        for (int k : {3, 4, 8}) {
            EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs.data(), end.data(), 0), SILENT_OK);
            EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs_h.data(), end_h.data(), 1), SILENT_OK);
            for (unsigned parts : {3u, 1u, 2u}) {
                EXPECT(GRAY_PASS_DEV(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs.data(), end.data(), 0, parts, nullptr), SILENT_OK);
                EXPECT(GRAY_PASS_DEV(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs_h.data(), end_h.data(), 1, parts, nullptr), SILENT_OK);
            }
#if SILENT_FRAME_BYTES == 4
            EXPECT(silent_gray_pass_dev(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs.data(), end.data(), nullptr), SILENT_OK);
            EXPECT(silent_gray_line_end(ctx, pyr.data(), extents, 3, n, cs_k, end_k, k, 255.0f, cs.data(), end.data()), SILENT_OK);
            EXPECT(silent_gray_line_end_dev(ctx, pyr.data(), extents, 3, n, cs_k, end_k, k, 255.0f, cs.data(), end.data(), nullptr), SILENT_OK);
#endif
        }
        EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), nullptr, end.data(), 0), SILENT_OK);
        EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), cs_h.data(), nullptr, 1), SILENT_OK);
        for (int sel = 0; sel < 2; ++sel) {
            // (no kernel runs in this build: the counts are whatever the staging arena held, so CAPACITY is as good as OK here)
            const int rc = FN(silent_gray_keypoints)(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), cs.data(), end.data(), 2, sel, 0.1,
                                                     regions, value.data(), sel ? peak.data() : nullptr, idx.data(), px, counts.data());
            if (rc != SILENT_OK && rc != SILENT_E_CAPACITY) {
                std::printf(NAME(silent_gray_keypoints) " (selection %d) -> %d (%s)\n", sel, rc, silent_last_error(ctx));
                ++failures;
            }
            EXPECT(FN_DEV(silent_gray_keypoints)(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), cs.data(), end.data(), 2, sel, 0.1,
                                                 regions, value.data(), sel ? peak.data() : nullptr, idx.data(), px, counts.data(), nullptr),
                   SILENT_OK);
        }
        // ---- status codes
        EXPECT(FN(silent_pyramid)(ctx, nullptr, frames, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(FN(silent_pyramid)(ctx, p, nullptr, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(FN(silent_pyramid)(ctx, p, frames, n, nullptr), SILENT_E_INVALID);
        EXPECT(FN(silent_pyramid)(ctx, p, frames, 0, pyr.data()), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_pyramid)(ctx, nullptr, frames, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_pyramid)(ctx, p, nullptr, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_pyramid)(ctx, p, frames, n, nullptr, nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_pyramid)(ctx, p, frames, 0, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_pyramid)(ctx, plan_other, frames, n, pyr.data(), nullptr), SILENT_E_INVALID);
#if SILENT_FRAME_BYTES != 4   // (silent_pyramid takes 3-channel and F64 plans)
        EXPECT(FN(silent_pyramid)(ctx, plan_rgb, frames, n, pyr.data()), SILENT_E_UNSUPPORTED);
        EXPECT(FN_DEV(silent_pyramid)(ctx, plan_rgb, frames, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
        EXPECT(FN(silent_pyramid)(ctx, plan_f64, frames, n, pyr.data()), SILENT_E_UNSUPPORTED);
        EXPECT(FN_DEV(silent_pyramid)(ctx, plan_f64, frames, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
#endif
        for (int f16 = 0; f16 < 2; ++f16) {
            void* c = f16 ? (void*)cs_h.data() : (void*)cs.data();
            void* e = f16 ? (void*)end_h.data() : (void*)end.data();
            EXPECT(GRAY_PASS(ctx, nullptr, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_INVALID);
            EXPECT(GRAY_PASS(ctx, p, nullptr, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_INVALID);
            EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, K, 255.0f, nullptr, c, e, f16), SILENT_E_INVALID);
            EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), nullptr, nullptr, f16), SILENT_E_INVALID);
            EXPECT(GRAY_PASS(ctx, p, frames, 0, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_INVALID);
            EXPECT(GRAY_PASS(ctx, plan_rgb, frames_rgb, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), WANT_RGB(f16));
            const bool f64_fits = WANT_F64(f16) != SILENT_OK || p == plan;   // plan_f64 is a ladder: a call that runs needs the ladder's maps
            if (f64_fits) EXPECT(GRAY_PASS(ctx, plan_f64, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), WANT_F64(f16));
            EXPECT(GRAY_PASS(ctx, p, frames, n, cs_k, end_k, 5, 255.0f, pyr.data(), c, e, f16), SILENT_E_UNSUPPORTED);
            EXPECT(GRAY_PASS_DEV(ctx, nullptr, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, p, nullptr, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, p, frames, n, cs_k, end_k, K, 255.0f, nullptr, c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), nullptr, nullptr, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, p, frames, 0, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 0u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, plan_other, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(GRAY_PASS_DEV(ctx, plan_rgb, frames_rgb, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), WANT_RGB(f16));
            if (f64_fits) EXPECT(GRAY_PASS_DEV(ctx, plan_f64, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), WANT_F64(f16));
            EXPECT(GRAY_PASS_DEV(ctx, p, frames, n, cs_k, end_k, 5, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_UNSUPPORTED);
        }
#define KP_ARGS(plan_, frames_, n_, k_) \
    ctx, plan_, frames_, n_, cs_k, end_k, k_, 255.0f, pyr.data(), cs.data(), end.data(), 2, 1, 0.1, regions, nullptr, nullptr, idx.data(), px, counts.data()
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(nullptr, frames, n, K)), SILENT_E_INVALID);
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(p, nullptr, n, K)), SILENT_E_INVALID);
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(p, frames, 0, K)), SILENT_E_INVALID);
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(plan_other, frames, n, K)), SILENT_E_INVALID);
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(plan_rgb, frames_rgb, n, K)), WANT_RGB(0));
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(p, frames, n, 5)), SILENT_E_UNSUPPORTED);
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(nullptr, frames, n, K), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(p, nullptr, n, K), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(p, frames, 0, K), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(plan_other, frames, n, K), nullptr), SILENT_E_INVALID);
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(plan_rgb, frames_rgb, n, K), nullptr), WANT_RGB(0));
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(p, frames, n, 5), nullptr), SILENT_E_UNSUPPORTED);
#if SILENT_FRAME_BYTES != 4   // (the float32-frame keypoint pass takes F64 plans)
        EXPECT(FN(silent_gray_keypoints)(KP_ARGS(plan_f64, frames, n, K)), SILENT_E_UNSUPPORTED);
        EXPECT(FN_DEV(silent_gray_keypoints)(KP_ARGS(plan_f64, frames, n, K), nullptr), SILENT_E_UNSUPPORTED);
#endif
#undef KP_ARGS
    }
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    std::free(frames);
    if (kFloatFrames) std::free(frames_rgb);
    for (silent_pyramid_plan* q : {plan, plan_crop, plan_rgb, plan_f64, plan_other}) silent_pyramid_plan_destroy(q);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    if (!refusals) std::printf("gray %s host main ok\n", SILENT_FRAME_BYTES == 4 ? "float32" : SILENT_FRAME_BYTES == 3 ? "rgb8" : "uint8");
    return 0;
}
