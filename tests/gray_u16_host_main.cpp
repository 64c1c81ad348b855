// Stand-alone driver of the uint16 entry points (silent_pyramid_u16, silent_gray_pass_u16, silent_gray_keypoints_u16, their *_view16 twins
// and the _dev forms: twelve) on the library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("u16")).  ONE translation unit
// with silent_unity.hip, -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel launches are compiled out and device memory is
// host memory, so what runs is the argument validation, the choice of the frame kind and the host forms' staging.  Every batch lies in a
// heap block of EXACTLY its span, (n - 1) * frame_stride + (H - 1) * row_stride + (W - 1) * pixel_stride + 2 bytes (2 * n * H * W for the
// packed entry points): a host form that stages one byte more reads past it (AddressSanitizer reports it).  No argument: every entry
// point on every layout + the status codes, one "ok" line.  --refusals: "name | case | status | silent_last_error" per (entry point,
// single fault), tests/golden/gray_u16_refusals.txt.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
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

constexpr int H = 40, W = 57, K = 4;

// a view of n frames in a heap block of exactly its span (strides in bytes)
struct Layout {
    const char* name;
    int n;
    int64_t pixel, row, frame;
};
static int64_t span_of(const Layout& l) { return (l.n - 1) * l.frame + (H - 1) * l.row + (W - 1) * l.pixel + 2; }
static const Layout kLayouts[] = {
    {"packed", 2, 2, 2 * W, 2 * H * W},
    {"pitched P010 luma", 2, 2, 128, 128 * H * 3 / 2},
    {"window of a larger frame, odd pitch in elements", 2, 2, 2 * 389, 2 * 389 * 163},
    {"every second element", 2, 4, 4 * W, 4 * W * H},
    {"one channel of 16-bit RGBA", 2, 8, 8 * W, 8 * W * H},
    {"every second frame", 2, 2, 2 * W, 4 * H * W},
    {"rows two bytes apart from packed", 2, 2, 2 * W + 2, (2 * W + 2) * H + 2},
    {"one frame, frame_stride not read", 1, 4, 4 * W + 6, 0},
    {"one frame, odd frame_stride not read", 1, 2, 2 * W, -1},
};

// ------------------------------------------------------------------------------------------ the refusal table
struct Args {
    silent_ctx* ctx; silent_pyramid_plan* plan; const uint16_t* frames; const silent_frame_view16* view; int n, k;
    const float *cs_k, *end_k;
    float *pyr, *cs, *end, *peak, *spare;
    unsigned parts; int pad, sel; const silent_extent* regions; int64_t *idx, *counts; size_t cap;
};
typedef uint64_t mask;
#define BIT(i) ((mask)1 << (i))
enum : mask {
    PLAN = BIT(0), FRAMES = BIT(1), PYR = BIT(2), CSK = BIT(3), BOTH = BIT(4), ENDBANK = BIT(5), N0 = BIT(6), K5 = BIT(7),
    OTHER = BIT(8), RGB = BIT(9), F64 = BIT(10), PARTS0 = BIT(11), REGIONS = BIT(12), COUNTS = BIT(13), IDX = BIT(14),
    PADNEG = BIT(15), SEL2 = BIT(16), PEAK0 = BIT(17),
    ODD_FRAMES = BIT(18),
    DATA = BIT(19), DATA_ODD = BIT(20), PX_LOW = BIT(21), PX_ODD = BIT(22), PX_ZERO = BIT(23), PX_NEG = BIT(24), ROW_LOW = BIT(25),
    ROW_ODD = BIT(26), ROW_ZERO = BIT(27), ROW_NEG = BIT(28), FRAME_LOW = BIT(29), FRAME_ODD = BIT(30), FRAME_ZERO = BIT(31),
    FRAME_NEG = BIT(32), SPAN = BIT(33)
};
constexpr int kFaults = 34;
constexpr mask kViewFaults = DATA | DATA_ODD | PX_LOW | PX_ODD | PX_ZERO | PX_NEG | ROW_LOW | ROW_ODD | ROW_ZERO | ROW_NEG | FRAME_LOW | FRAME_ODD |
                             FRAME_ZERO | FRAME_NEG | SPAN;
static const char* const kFaultNames[kFaults] = {
    "plan NULL", "frames / view NULL", "pyr NULL", "cs_kernel NULL", "both map outputs NULL", "end_out without end_bank", "n_frames 0", "n_orient 5",
    "plan of another context", "3-channel plan", "ACCUM_F64 plan", "parts 0", "regions NULL", "counts NULL", "idx NULL with a cap", "pad -1",
    "selection 2", "peak_value_out with selection 0",
    "frames at an odd address",
    "data NULL", "data at an odd address", "pixel_stride 1", "pixel_stride odd", "pixel_stride 0", "pixel_stride -4", "row_stride one below its bound",
    "row_stride odd", "row_stride 0", "row_stride negative", "frame_stride one below its bound", "frame_stride odd", "frame_stride 0",
    "frame_stride negative", "frame_stride 2^63 - 2 (a span of 2^63 bytes or more)"};
struct Entry {
    const char* name;
    bool view;
    mask faults;
    std::function<int(const Args&)> call;
};
#define KP_TAIL(a) a.n, a.cs_k, a.end_k, a.k, 65535.0f, a.pyr, a.cs, a.end, a.pad, a.sel, 0.1, a.regions, nullptr, a.peak, a.idx, a.cap, a.counts
#define GP_TAIL(a) a.n, a.cs_k, a.end_k, a.k, 65535.0f, a.pyr
static std::vector<Entry> entries() {
    const mask pyr = PLAN | FRAMES | PYR | N0 | RGB | F64;
    const mask gp = PLAN | FRAMES | PYR | CSK | BOTH | ENDBANK | N0 | K5 | RGB | F64;
    // (the host form of the keypoint pass takes NULL pyr / cs_out / end_out: the maps then live in the staging arena)
    const mask kp = PLAN | FRAMES | CSK | ENDBANK | N0 | K5 | RGB | F64 | REGIONS | COUNTS | IDX | PADNEG | SEL2 | PEAK0;
    const mask u = ODD_FRAMES, v = kViewFaults;
    std::vector<Entry> e;
    e.push_back({"silent_pyramid_u16", false, pyr | u, [](const Args& a) { return silent_pyramid_u16(a.ctx, a.plan, a.frames, a.n, a.pyr); }});
    e.push_back({"silent_pyramid_u16_dev", false, pyr | u | OTHER, [](const Args& a) { return silent_pyramid_u16_dev(a.ctx, a.plan, a.frames, a.n, a.pyr, nullptr); }});
    e.push_back({"silent_gray_pass_u16", false, gp | u, [](const Args& a) { return silent_gray_pass_u16(a.ctx, a.plan, a.frames, GP_TAIL(a), a.cs, a.end, 0); }});
    e.push_back({"silent_gray_pass_u16_dev", false, gp | u | OTHER | PARTS0,
                 [](const Args& a) { return silent_gray_pass_u16_dev(a.ctx, a.plan, a.frames, GP_TAIL(a), a.cs, a.end, 0, a.parts, nullptr); }});
    e.push_back({"silent_gray_keypoints_u16", false, kp | u, [](const Args& a) { return silent_gray_keypoints_u16(a.ctx, a.plan, a.frames, KP_TAIL(a)); }});
    e.push_back({"silent_gray_keypoints_u16_dev", false, kp | u | PYR | BOTH | OTHER,
                 [](const Args& a) { return silent_gray_keypoints_u16_dev(a.ctx, a.plan, a.frames, KP_TAIL(a), nullptr); }});
    e.push_back({"silent_pyramid_view16", true, pyr | v, [](const Args& a) { return silent_pyramid_view16(a.ctx, a.plan, a.view, a.n, a.pyr); }});
    e.push_back({"silent_pyramid_view16_dev", true, pyr | v | OTHER, [](const Args& a) { return silent_pyramid_view16_dev(a.ctx, a.plan, a.view, a.n, a.pyr, nullptr); }});
    e.push_back({"silent_gray_pass_view16", true, gp | v, [](const Args& a) { return silent_gray_pass_view16(a.ctx, a.plan, a.view, GP_TAIL(a), a.cs, a.end, 0); }});
    e.push_back({"silent_gray_pass_view16_dev", true, gp | v | OTHER | PARTS0,
                 [](const Args& a) { return silent_gray_pass_view16_dev(a.ctx, a.plan, a.view, GP_TAIL(a), a.cs, a.end, 0, a.parts, nullptr); }});
    e.push_back({"silent_gray_keypoints_view16", true, kp | v, [](const Args& a) { return silent_gray_keypoints_view16(a.ctx, a.plan, a.view, KP_TAIL(a)); }});
    e.push_back({"silent_gray_keypoints_view16_dev", true, kp | v | PYR | BOTH | OTHER,
                 [](const Args& a) { return silent_gray_keypoints_view16_dev(a.ctx, a.plan, a.view, KP_TAIL(a), nullptr); }});
    return e;
}

static void refusal_table(bool views, const Args& valid, silent_pyramid_plan* plan_other, silent_pyramid_plan* plan_rgb, silent_pyramid_plan* plan_f64) {
    for (const Entry& e : entries()) {
        if (e.view != views) continue;
        for (int f = 0; f < kFaults; ++f) {
            if (!(e.faults & BIT(f))) continue;
            Args a = valid;
            silent_frame_view16 v = *valid.view;
            a.view = &v;
            const int64_t row_min = (W - 1) * v.pixel_stride + 2, frame_min = (H - 1) * v.row_stride + row_min;
            const uint16_t* odd = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(valid.frames) + 1);   // (never dereferenced)
            switch (BIT(f)) {
                case PLAN: a.plan = nullptr; break;
                case FRAMES: a.frames = nullptr; a.view = nullptr; break;
                case PYR: a.pyr = nullptr; break;
                case CSK: a.cs_k = nullptr; break;
                case BOTH: a.cs = a.end = nullptr; break;
                case ENDBANK: a.end_k = nullptr; break;
                case N0: a.n = 0; break;                   case K5: a.k = 5; break;
                case OTHER: a.plan = plan_other; break;    case F64: a.plan = plan_f64; break;
                case RGB: a.plan = plan_rgb; break;
                case PARTS0: a.parts = 0u; break;          case REGIONS: a.regions = nullptr; break;
                case COUNTS: a.counts = nullptr; break;    case IDX: a.idx = nullptr; break;
                case PADNEG: a.pad = -1; break;            case SEL2: a.sel = 2; break;
                case PEAK0: a.sel = 0; a.peak = a.spare; break;
                case ODD_FRAMES: a.frames = odd; break;
                case DATA: v.data = nullptr; break;        case DATA_ODD: v.data = odd; break;
                case PX_LOW: v.pixel_stride = 1; break;    case PX_ODD: v.pixel_stride += 1; break;
                case PX_ZERO: v.pixel_stride = 0; break;   case PX_NEG: v.pixel_stride = -4; break;
                case ROW_LOW: v.row_stride = row_min - 1; break;
                case ROW_ODD: v.row_stride += 1; break;
                case ROW_ZERO: v.row_stride = 0; break;    case ROW_NEG: v.row_stride = -v.row_stride; break;
                case FRAME_LOW: v.frame_stride = frame_min - 1; break;
                case FRAME_ODD: v.frame_stride += 1; break;
                case FRAME_ZERO: v.frame_stride = 0; break; case FRAME_NEG: v.frame_stride = -v.frame_stride; break;
                case SPAN: v.frame_stride = INT64_MAX - 1; break;
            }
            const int rc = e.call(a);
            std::printf("%s | %s | %d | %s\n", e.name, kFaultNames[f], rc, rc == SILENT_OK ? "-" : silent_last_error(a.ctx));
        }
    }
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
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

    float cs_k[9], end_k[9 * 8];
    for (int i = 0; i < 9; ++i) cs_k[i] = i == 4 ? 1.0f : -0.125f;
    for (int i = 0; i < 9 * 8; ++i) end_k[i] = (float)((i % 5) - 2) * 0.25f;

    silent_pyramid_plan* plans[2] = {plan, plan_crop};
    for (silent_pyramid_plan* p : plans) {
        const size_t px = (size_t)2 * (p == plan ? 40 * 57 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
        std::vector<float> pyr(px), cs(px), end(px * 8), value(px), peak(px);
        std::vector<uint16_t> cs_h(px), end_h(px * 8);
        std::vector<int64_t> idx(2 * px * 4), counts(2);
        silent_extent regions[3];
        const silent_pyr_level* lv = p == plan ? ladder : crops;
        for (int l = 0; l < 3; ++l) regions[l] = silent_extent{lv[l].out_h / 2 > 0 ? lv[l].out_h / 2 : 1, lv[l].out_w / 2 > 0 ? lv[l].out_w / 2 : 1};
        for (const Layout& lay : kLayouts) {
            const size_t span = (size_t)span_of(lay);
            uint16_t* block = (uint16_t*)std::malloc(span);          // exactly the span: not one byte more
            for (size_t i = 0; i < span / 2; ++i) block[i] = (uint16_t)(i * 3701 + 1117);
            const silent_frame_view16 view = {block, lay.pixel, lay.row, lay.frame};
            const int n = lay.n;
            const bool packed = !std::strcmp(lay.name, "packed");
            if (refusals) {
                // the packed entry points on the packed block, the view entry points on one strided layout; two frames (so every stride is read)
                if (p == plan && (packed || !std::strcmp(lay.name, "pitched P010 luma"))) {
                    std::printf("# %s\n", lay.name);
                    refusal_table(!packed, Args{ctx, p, block, &view, n, K, cs_k, end_k, pyr.data(), cs.data(), end.data(), nullptr, peak.data(), 3u, 2, 1,
                                                regions, idx.data(), counts.data(), px},
                                  plan_other, plan_rgb, plan_f64);
                }
                std::free(block);
                continue;
            }
            // ---- every view entry point, host and _dev form (device memory is host memory here)
            EXPECT(silent_pyramid_view16(ctx, p, &view, n, pyr.data()), SILENT_OK);
            EXPECT(silent_pyramid_view16_dev(ctx, p, &view, n, pyr.data(), nullptr), SILENT_OK);
            for (int k : {3, 4, 8}) {
                EXPECT(silent_gray_pass_view16(ctx, p, &view, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs.data(), end.data(), 0), SILENT_OK);
                EXPECT(silent_gray_pass_view16(ctx, p, &view, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs_h.data(), end_h.data(), 1), SILENT_OK);
                for (unsigned parts : {3u, 1u, 2u}) {
                    EXPECT(silent_gray_pass_view16_dev(ctx, p, &view, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs.data(), end.data(), 0, parts, nullptr),
                           SILENT_OK);
                    EXPECT(silent_gray_pass_view16_dev(ctx, p, &view, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs_h.data(), end_h.data(), 1, parts, nullptr),
                           SILENT_OK);
                }
            }
            EXPECT(silent_gray_pass_view16(ctx, p, &view, n, cs_k, end_k, K, 65535.0f, pyr.data(), nullptr, end.data(), 0), SILENT_OK);
            EXPECT(silent_gray_pass_view16(ctx, p, &view, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs_h.data(), nullptr, 1), SILENT_OK);
            for (int sel = 0; sel < 2; ++sel) {
                // (no kernel runs in this build: the counts are whatever the staging arena held, so CAPACITY is as good as OK here)
                const int rc = silent_gray_keypoints_view16(ctx, p, &view, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 2, sel, 0.1,
                                                            regions, value.data(), sel ? peak.data() : nullptr, idx.data(), px, counts.data());
                if (rc != SILENT_OK && rc != SILENT_E_CAPACITY) {
                    std::printf("silent_gray_keypoints_view16 (%s, selection %d) -> %d (%s)\n", lay.name, sel, rc, silent_last_error(ctx));
                    ++failures;
                }
                EXPECT(silent_gray_keypoints_view16_dev(ctx, p, &view, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 2, sel, 0.1, regions,
                                                        value.data(), sel ? peak.data() : nullptr, idx.data(), px, counts.data(), nullptr),
                       SILENT_OK);
            }
            // ---- the packed entry points on the packed block: exactly 2 * n * H * W bytes
            if (packed) {
                EXPECT(silent_pyramid_u16(ctx, p, block, n, pyr.data()), SILENT_OK);
                EXPECT(silent_pyramid_u16_dev(ctx, p, block, n, pyr.data(), nullptr), SILENT_OK);
                for (int k : {3, 4, 8}) {
                    EXPECT(silent_gray_pass_u16(ctx, p, block, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs.data(), end.data(), 0), SILENT_OK);
                    EXPECT(silent_gray_pass_u16(ctx, p, block, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs_h.data(), end_h.data(), 1), SILENT_OK);
                    for (unsigned parts : {3u, 1u, 2u})
                        EXPECT(silent_gray_pass_u16_dev(ctx, p, block, n, cs_k, end_k, k, 65535.0f, pyr.data(), cs_h.data(), end_h.data(), 1, parts, nullptr),
                               SILENT_OK);
                }
                const int rc = silent_gray_keypoints_u16(ctx, p, block, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 2, 1, 0.1, regions,
                                                         value.data(), peak.data(), idx.data(), px, counts.data());
                if (rc != SILENT_OK && rc != SILENT_E_CAPACITY) {
                    std::printf("silent_gray_keypoints_u16 -> %d (%s)\n", rc, silent_last_error(ctx));
                    ++failures;
                }
                EXPECT(silent_gray_keypoints_u16_dev(ctx, p, block, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 2, 0, 0.1, regions,
                                                     value.data(), nullptr, idx.data(), px, counts.data(), nullptr),
                       SILENT_OK);
                const uint16_t* odd = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(block) + 1);
                EXPECT(silent_pyramid_u16(ctx, p, odd, n, pyr.data()), SILENT_E_INVALID);
                EXPECT(silent_pyramid_u16(ctx, plan_rgb, block, n, pyr.data()), SILENT_E_UNSUPPORTED);
                EXPECT(silent_gray_pass_u16_dev(ctx, plan_f64, block, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 0, 3u, nullptr),
                       SILENT_E_UNSUPPORTED);
            }
            // ---- status codes: what the *_u16 forms refuse, and the view's own refusals
            silent_frame_view16 bad = view;
            EXPECT(silent_pyramid_view16(ctx, p, nullptr, n, pyr.data()), SILENT_E_INVALID);
            EXPECT(silent_pyramid_view16(ctx, plan_rgb, &view, n, pyr.data()), SILENT_E_UNSUPPORTED);
            EXPECT(silent_pyramid_view16_dev(ctx, plan_f64, &view, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_view16(ctx, p, &view, n, cs_k, end_k, 5, 65535.0f, pyr.data(), cs.data(), end.data(), 0), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_view16_dev(ctx, plan_other, &view, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 0, 3u, nullptr),
                   SILENT_E_INVALID);
            bad.pixel_stride = view.pixel_stride + 1;
            EXPECT(silent_gray_pass_view16_dev(ctx, p, &bad, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 0, 3u, nullptr), SILENT_E_INVALID);
            bad = view;
            bad.row_stride = (W - 1) * view.pixel_stride;
            EXPECT(silent_pyramid_view16(ctx, p, &bad, n, pyr.data()), SILENT_E_INVALID);
            bad = view;
            bad.data = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(block) + 1);
            EXPECT(silent_gray_keypoints_view16(ctx, p, &bad, n, cs_k, end_k, K, 65535.0f, pyr.data(), cs.data(), end.data(), 2, 1, 0.1, regions, nullptr,
                                                nullptr, idx.data(), px, counts.data()),
                   SILENT_E_INVALID);
            if (n > 1) {
                bad = view;
                bad.frame_stride = (H - 1) * view.row_stride + (W - 1) * view.pixel_stride;
                EXPECT(silent_pyramid_view16_dev(ctx, p, &bad, n, pyr.data(), nullptr), SILENT_E_INVALID);
            }
            std::free(block);
        }
    }
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    for (silent_pyramid_plan* q : {plan, plan_crop, plan_rgb, plan_f64, plan_other}) silent_pyramid_plan_destroy(q);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    if (!refusals) std::printf("gray u16 host main ok\n");
    return 0;
}
