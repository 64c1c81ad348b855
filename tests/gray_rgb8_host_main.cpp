// Stand-alone driver of the interleaved-colour uint8-frame entry points (silent_*_u8x3) on the library's HOST side
// (tests/test_gray_rgb8_host.py compiles it as ONE
// translation unit with pysilent_amd/csrc/silent_unity.hip -- included below --, -DSILENT_HOST_ONLY, under
// -fsanitize=address,undefined, and runs the executable).
// In that build kernel launches are compiled out and device memory is host memory, so what runs is the argument validation, the
// plan tables and the host-pointer forms' staging.  The colour frames are heap blocks of EXACTLY 3 * n * H * W bytes: a staging size
// written as "* 4" reads past them, which AddressSanitizer reports (and one written without the "3 *" is caught by the GPU tests).
// The plans are SINGLE-CHANNEL plans: the frame layout is a property of the call.  Prints one "ok" line.
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

int main() {
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

    uint8_t* frames = (uint8_t*)std::malloc((size_t)3 * n * H * W);   // exactly 3 * n * H * W bytes
    for (int i = 0; i < 3 * n * H * W; ++i) frames[i] = (uint8_t)(i * 37 + 11);
    float cs_k[9], end_k[9 * 8];
    for (int i = 0; i < 9; ++i) cs_k[i] = i == 4 ? 1.0f : -0.125f;
    for (int i = 0; i < 9 * 8; ++i) end_k[i] = (float)((i % 5) - 2) * 0.25f;

    silent_pyramid_plan* plans[2] = {plan, plan_crop};
    for (silent_pyramid_plan* p : plans) {
        const size_t px = (size_t)n * (p == plan ? 40 * 57 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
        std::vector<float> pyr(px), cs(px), end(px * 8), value(px), peak(px);
        std::vector<uint16_t> cs_h(px), end_h(px * 8);
        std::vector<int64_t> idx(n * px * 4), counts(n);
        silent_extent regions[3];
        const silent_pyr_level* lv = p == plan ? ladder : crops;
        for (int l = 0; l < 3; ++l) regions[l] = silent_extent{lv[l].out_h / 2 > 0 ? lv[l].out_h / 2 : 1, lv[l].out_w / 2 > 0 ? lv[l].out_w / 2 : 1};
        // ---- every new entry point, host and _dev form (device memory is host memory here)
        EXPECT(silent_pyramid_u8x3(ctx, p, frames, n, pyr.data()), SILENT_OK);
        EXPECT(silent_pyramid_u8x3_dev(ctx, p, frames, n, pyr.data(), nullptr), SILENT_OK);
        for (int k : {3, 4, 8}) {
            EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs.data(), end.data(), 0), SILENT_OK);
            EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs_h.data(), end_h.data(), 1), SILENT_OK);
            for (unsigned parts : {3u, 1u, 2u}) {
                EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs.data(), end.data(), 0, parts, nullptr), SILENT_OK);
                EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, n, cs_k, end_k, k, 255.0f, pyr.data(), cs_h.data(), end_h.data(), 1, parts, nullptr), SILENT_OK);
            }
        }
        EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), nullptr, end.data(), 0), SILENT_OK);
        EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), cs_h.data(), nullptr, 1), SILENT_OK);
        for (int sel = 0; sel < 2; ++sel) {
            // (no kernel runs in this build: the counts are whatever the staging arena held, so CAPACITY is as good as OK here)
            const int rc = silent_gray_keypoints_u8x3(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), cs.data(), end.data(), 2, sel, 0.1,
                                                    regions, value.data(), sel ? peak.data() : nullptr, idx.data(), px, counts.data());
            if (rc != SILENT_OK && rc != SILENT_E_CAPACITY) {
                std::printf("silent_gray_keypoints_u8x3 (selection %d) -> %d (%s)\n", sel, rc, silent_last_error(ctx));
                ++failures;
            }
            EXPECT(silent_gray_keypoints_u8x3_dev(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), cs.data(), end.data(), 2, sel, 0.1,
                                                regions, value.data(), sel ? peak.data() : nullptr, idx.data(), px, counts.data(), nullptr),
                   SILENT_OK);
        }
        // ---- status codes
        EXPECT(silent_pyramid_u8x3(ctx, nullptr, frames, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3(ctx, p, nullptr, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3(ctx, p, frames, n, nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3(ctx, p, frames, 0, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3_dev(ctx, nullptr, frames, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3_dev(ctx, p, nullptr, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3_dev(ctx, p, frames, n, nullptr, nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3_dev(ctx, p, frames, 0, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3_dev(ctx, plan_other, frames, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_u8x3(ctx, plan_rgb, frames, n, pyr.data()), SILENT_E_UNSUPPORTED);
        EXPECT(silent_pyramid_u8x3_dev(ctx, plan_rgb, frames, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
        EXPECT(silent_pyramid_u8x3(ctx, plan_f64, frames, n, pyr.data()), SILENT_E_UNSUPPORTED);
        EXPECT(silent_pyramid_u8x3_dev(ctx, plan_f64, frames, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
        for (int f16 = 0; f16 < 2; ++f16) {
            void* c = f16 ? (void*)cs_h.data() : (void*)cs.data();
            void* e = f16 ? (void*)end_h.data() : (void*)end.data();
            EXPECT(silent_gray_pass_u8x3(ctx, nullptr, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3(ctx, p, nullptr, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, K, 255.0f, nullptr, c, e, f16), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), nullptr, nullptr, f16), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3(ctx, p, frames, 0, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3(ctx, plan_rgb, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_u8x3(ctx, plan_f64, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_u8x3(ctx, p, frames, n, cs_k, end_k, 5, 255.0f, pyr.data(), c, e, f16), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, nullptr, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, p, nullptr, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, n, cs_k, end_k, K, 255.0f, nullptr, c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), nullptr, nullptr, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, 0, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 0u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, plan_other, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_INVALID);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, plan_rgb, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, plan_f64, frames, n, cs_k, end_k, K, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_UNSUPPORTED);
            EXPECT(silent_gray_pass_u8x3_dev(ctx, p, frames, n, cs_k, end_k, 5, 255.0f, pyr.data(), c, e, f16, 3u, nullptr), SILENT_E_UNSUPPORTED);
        }
#define KP_ARGS(plan_, frames_, n_, k_) \
    ctx, plan_, frames_, n_, cs_k, end_k, k_, 255.0f, pyr.data(), cs.data(), end.data(), 2, 1, 0.1, regions, nullptr, nullptr, idx.data(), px, counts.data()
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(nullptr, frames, n, K)), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(p, nullptr, n, K)), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(p, frames, 0, K)), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(plan_other, frames, n, K)), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(plan_rgb, frames, n, K)), SILENT_E_UNSUPPORTED);
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(plan_f64, frames, n, K)), SILENT_E_UNSUPPORTED);
        EXPECT(silent_gray_keypoints_u8x3(KP_ARGS(p, frames, n, 5)), SILENT_E_UNSUPPORTED);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(nullptr, frames, n, K), nullptr), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(p, nullptr, n, K), nullptr), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(p, frames, 0, K), nullptr), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(plan_other, frames, n, K), nullptr), SILENT_E_INVALID);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(plan_rgb, frames, n, K), nullptr), SILENT_E_UNSUPPORTED);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(plan_f64, frames, n, K), nullptr), SILENT_E_UNSUPPORTED);
        EXPECT(silent_gray_keypoints_u8x3_dev(KP_ARGS(p, frames, n, 5), nullptr), SILENT_E_UNSUPPORTED);
#undef KP_ARGS
    }
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    std::free(frames);
    silent_pyramid_plan_destroy(plan);
    silent_pyramid_plan_destroy(plan_crop);
    silent_pyramid_plan_destroy(plan_rgb);
    silent_pyramid_plan_destroy(plan_f64);
    silent_pyramid_plan_destroy(plan_other);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("gray rgb8 host main ok\n");
    return 0;
}
